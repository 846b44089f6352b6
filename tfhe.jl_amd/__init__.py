"""tfhe.jl_amd — MI355X-native TFHE gate bootstrapping behind the reference's gate_*/key API.

Exports mirror src/TFHE.jl:24-61 of nucypher/TFHE.jl.  The hot path (gate_* -> bootstrap ->
keyswitch) runs in hand-written HIP kernels (csrc/, C ABI in include/tfhe_mi355x.h); key generation,
encryption and decryption stay on the host, as in the reference.
"""
from .params import (SchemeParameters, tfhe_parameters_80, tfhe_parameters_128,
                     mktfhe_parameters_2party, mktfhe_parameters_4party, mktfhe_parameters_8party)
from .lwe import LweSample, LweSampleArray
from .keys import SecretKey, CloudKey, make_key_pair, encrypt, decrypt
from .gates import (gate_nand, gate_or, gate_and, gate_xor, gate_xnor, gate_not, gate_constant, gate_nor,
                    gate_andny, gate_andyn, gate_orny, gate_oryn, gate_mux, gates_batch)
from .mk_keys import SharedKey, CloudKeyPart, MKCloudKey, MKLweSample, mk_encrypt, mk_decrypt, mk_gate_nand
from .mk_gates import (mk_gate_or, mk_gate_and, mk_gate_xor, mk_gate_xnor, mk_gate_nor, mk_gate_andny, mk_gate_andyn,
                       mk_gate_orny, mk_gate_oryn, mk_gate_mux, mk_gate_not, mk_gate_constant, mk_gates_batch)
from .circuit import Circuit
from .lut import (lut_encode, lut_decode, lut_encrypt, lut_decrypt, make_test_vector, programmable_bootstrap, make_multi_test_vector,
                  programmable_bootstrap_multi, make_gate_test_vector, GATE_BIT_TO_Z2)
from .serialize import save_cloud_key, load_cloud_key
from .leveled import tlwe_encrypt, tlwe_trivial, tlwe_phase, tgsw_encrypt_bits, table_to_tlwe, cmux_lookup
from .leveled import CmuxNet, tree_net, dfa_net, less_than_net, cmux_net_lookup
from .leveled import RotNet, pack_table_to_tlwe, packed_lookup_net, wfa_net, rot_net_lookup, packed_lookup
from .leveled import mk_tlwe_trivial, mk_tlwe_encrypt, mk_tlwe_phase, mk_tgsw_uni_encrypt_bits, mk_tgsw_expand, mk_cmux_lookup, mk_cmux_net_lookup
from .leveled import packed_words_net, pack_words_to_tlwe, mk_rot_net_lookup, mk_packed_lookup
from .leveled import bootstrap_key_selectors, private_lut_encrypt, blind_rotate_lookup, two_stage_lookup, pbs_to_tlwe
from .leveled import mk_bootstrap_key_selectors, mk_private_lut_encrypt, mk_blind_rotate_lookup, mk_two_stage_lookup, mk_pbs_to_tlwe
from .leveled import mk_two_stage_lookup_device
from ._lib import Engine, EngineError, OPCODES, LIB_PATH, pinned_empty

__all__ = [
    "make_key_pair", "LweSample", "LweSampleArray", "SecretKey", "CloudKey", "encrypt", "decrypt",
    "tfhe_parameters_80", "tfhe_parameters_128", "SchemeParameters",
    "gate_nand", "gate_or", "gate_and", "gate_xor", "gate_xnor", "gate_not", "gate_constant", "gate_nor",
    "gate_andny", "gate_andyn", "gate_orny", "gate_oryn", "gate_mux", "gates_batch",
    "mktfhe_parameters_2party", "mktfhe_parameters_4party", "mktfhe_parameters_8party",
    "SharedKey", "CloudKeyPart", "MKCloudKey", "MKLweSample", "mk_encrypt", "mk_decrypt", "mk_gate_nand",
    "mk_gate_or", "mk_gate_and", "mk_gate_xor", "mk_gate_xnor", "mk_gate_nor", "mk_gate_andny", "mk_gate_andyn",
    "mk_gate_orny", "mk_gate_oryn", "mk_gate_mux", "mk_gate_not", "mk_gate_constant", "mk_gates_batch",
    "Circuit", "lut_encode", "lut_decode", "lut_encrypt", "lut_decrypt", "make_test_vector", "programmable_bootstrap",
    "make_multi_test_vector", "programmable_bootstrap_multi", "make_gate_test_vector", "GATE_BIT_TO_Z2",
    "tlwe_encrypt", "tlwe_trivial", "tlwe_phase", "tgsw_encrypt_bits", "table_to_tlwe", "cmux_lookup",
    "CmuxNet", "tree_net", "dfa_net", "less_than_net", "cmux_net_lookup",
    "RotNet", "pack_table_to_tlwe", "packed_lookup_net", "wfa_net", "rot_net_lookup", "packed_lookup",
    "packed_words_net", "pack_words_to_tlwe", "mk_rot_net_lookup", "mk_packed_lookup",
    "bootstrap_key_selectors", "private_lut_encrypt", "blind_rotate_lookup", "two_stage_lookup", "pbs_to_tlwe",
    "mk_bootstrap_key_selectors", "mk_private_lut_encrypt", "mk_blind_rotate_lookup", "mk_two_stage_lookup", "mk_pbs_to_tlwe",
    "mk_two_stage_lookup_device",
    "save_cloud_key", "load_cloud_key", "Engine", "EngineError", "OPCODES", "LIB_PATH", "pinned_empty",
]
