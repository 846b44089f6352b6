"""CMUX networks under a multi-key cloud key (tfhe_mk_cmux_net_batch; Engine.mk_cmux_net, tfhe_jl_amd.leveled.mk_cmux_net_lookup) against
an integer schoolbook network.

The reference of every word comparison is `mk_net_ref` below: tests/test_mk_leveled.py's `MKTree.cmux` (exact int64, np.convolve, no
transform, no rounding) per node, a copy node copying, then `MKTree.extract` and `MKTree.keyswitch` — never the engine.  There are no
tolerances: sums of spectra and sums of integer products are the same integers where the set is exact.

Noise (why "all 8 comparisons correct" at full size is a condition, not a measurement): the comparator's accepting path crosses at most
one non-copy node per level, 32 levels for 16-bit operands, each adding one multi-key external product's noise (1.8e-3 of the torus at
mktfhe_parameters_2party, tests/test_mk_leveled.py) to a window of 1/8.  The schoolbook network alone gave 16 of 16 pairs there with the
worst phase error 1.1e-2 of the torus at coefficient 0 (x = y: a non-copy node on all 32 levels); the keyswitch adds about 3e-3.
"""
import ctypes as C
import os

import numpy as np
import pytest

from test_cmux_net import _mem_free, _ptr, random_net
from test_mk_leveled import MKTree, Setup, _gate_table, _words

INVALID, NO_KEY, STATE, NOMEM = 1, 3, 5, 6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mk_net_ref(ref, net, table, sels):
    """The schoolbook network: `ref` an MKTree over the selector set, `table` [E][P+1][N], sels[var] the selector behind each variable
    of the row.  Returns the outputs of the last level, int64 [F][P+1][N]."""
    cur = [np.asarray(t, np.int64) for t in table]
    for v in range(net.levels):
        cur = [cur[s0].copy() if s0 == s1 else ref.cmux(sels[var], cur[s0], cur[s1]) for s0, s1, var in net.level(v).tolist()]
    return np.stack(cur)


def ref_rows(ref, net, data, rows, sel, with_ks=False):
    """(samples [B][F][P+1][N], extracted [B][F][P N+1], keyswitched [B][F][P n+1] or None) of the schoolbook network, as int32."""
    want = np.stack([mk_net_ref(ref, net, data[rows[g]], sel[g]) for g in range(len(sel))])
    ext = np.stack([[ref.extract(w) for w in row] for row in want])
    ks = np.stack([[ref.keyswitch(e) for e in row] for row in ext]).astype(np.int32) if with_ks else None
    return want.astype(np.int32), ext.astype(np.int32), ks


def _compare_bits(x, y, d):
    return [(x >> b) & 1 for b in range(d)] + [(y >> b) & 1 for b in range(d)]


# ---- 1. CPU ------------------------------------------------------------------------------------------------------------------------
def test_new_symbol_is_declared_bound_and_exported(tfhe):
    name = "tfhe_mk_cmux_net_batch"
    header = open(os.path.join(ROOT, "include", "tfhe_mi355x.h")).read()
    lib = tfhe._lib.load()
    assert name in tfhe._lib.ABI_SYMBOLS and f"int32_t {name}(tfhe_ctx *ctx" in header and hasattr(lib, name)
    assert len(lib.tfhe_mk_cmux_net_batch.argtypes) == 13
    assert lib.tfhe_abi_version() == 7
    assert callable(tfhe.Engine.mk_cmux_net) and callable(tfhe.leveled.mk_cmux_net_lookup)


def test_schoolbook_network_decrypts_the_two_party_comparator(tfhe, orc):
    """(P, N, l, beta) = (2, 64, 3, 7): less_than_net(4) as a schoolbook network, party 0 uni-encrypting the bits of x and party 1 those
    of y, a trivial gate-encoded table: the phase at coefficient 0 (mk_tlwe_phase) has the sign of x < y and lies within 2^28 of
    +-2^29.  Measured through this schoolbook over the six pairs: the worst error is 2^25.3, the figure that test_mk_leveled's
    tree measured after three levels at this set (the error is dominated by single large terms, not by the number of levels)."""
    from tfhe_jl_amd import leveled
    P, N, l, beta, d = 2, 64, 3, 7, 4
    net, table = leveled.less_than_net(d)
    data = leveled.table_to_tlwe(table, N, k=P)
    assert data.shape == (5, P + 1, N) and not data[:, :P].any()
    worst = 0
    for x, y in [(5, 5), (5, 6), (5, 4), (0, 15), (15, 0), (9, 12)]:                      # x = y, y = x +- 1, the extremes, a mixed pair
        bits = _compare_bits(x, y, d)
        assert net.evaluate_clear(table, bits) == [x < y]
        s = Setup(tfhe, P, N, l, beta, 4100 + 16 * x + y, owners=[0] * d + [1] * d, bits=bits)
        got = mk_net_ref(s.tree(orc), net, data, list(range(2 * d)))
        assert got.shape == (1, P + 1, N)
        phase = leveled.mk_tlwe_phase(s.tlwe_keys, got[0].astype(np.int32))[0]
        err = abs(int(phase[0]) - (2**29 if x < y else -2**29))
        worst = max(worst, err)
        assert (phase[0] > 0) == (x < y), (x, y, phase[0])
        assert err < 2**28, (x, y, phase[0])
        s.ck.close()
    print(f"worst phase error at coefficient 0: 2^{np.log2(max(worst, 1)):.1f}")


# ---- 2. GPU: a random network word for word ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("P,N,l,beta", [(2, 64, 3, 7), (3, 32, 2, 8), (4, 64, 2, 10), (2, 1024, 4, 7)])
def test_gpu_mk_random_network_equals_schoolbook(tfhe, orc, P, N, l, beta):
    from tfhe_jl_amd import leveled
    B, T, E, V, widths = 3, 2, 5, 4, [4, 3, 2]
    owners = [0, 1, 2 % P, P - 1, 1, 0]                                  # every party owns a selector
    s = Setup(tfhe, P, N, l, beta, 6300 + P + N + l, owners)
    eng = s.ck.engine(0)
    data = s.encrypt(_words(s.rng, T * E, N)).reshape(T, E, P + 1, N)
    net = leveled.CmuxNet(widths, random_net(s.rng, E, widths, V), entries=E, variables=V)
    assert net.products == 7
    sel = np.array([[0, 1, 2, 3], [5, 4, 0, 2], [3, 3, 1, 5]], np.int32)    # rows differ; a selector behind two variables
    index = np.array([1, 0, 1], np.int32)
    lv0 = net.level(0)
    assert set(owners) == set(range(P)) and owners[sel[0, lv0[2, 2]]] != owners[sel[0, lv0[3, 2]]]      # level 0 of row 0 mixes parties
    if eng.get_option("exact_domain") == 2:                               # exact for ANY words: an arbitrary table with the extremes
        extra = _words(s.rng, 1, E, P + 1, N)
        extra[0, 1], extra[0, 2], extra[0, 3] = 2**31 - 1, -2**31, 0
        data = np.concatenate([data, extra])
        sel = np.concatenate([sel, np.array([[4, 2, 3, 1]], np.int32)])
        index = np.concatenate([index, np.array([2], np.int32)])
        B, T = B + 1, T + 1
    ref = s.tree(orc, with_ks=True)
    eng.mk_tgsw_load(s.tgsw, s.owners)
    for idx in (index, None):                                             # mixed tables, and NULL = table 0 for every row
        want, want_ext, want_ks = ref_rows(ref, net, data, [0] * B if idx is None else idx, sel, with_ks=True)
        got0 = eng.mk_cmux_net(data, net, sel, table_index=idx, out_form=0)
        assert got0.shape == (B, 2, P + 1, N) and np.array_equal(got0, want), ("out_form 0", idx)
        assert eng.last_kernel_name() == f"mk_cmux_net_level_kernel(N={N},P={P},l={l})"
        assert eng.last_rotation_count() == 0 and eng.last_timing_ms(0) > 0
        got1 = eng.mk_cmux_net(data, net, sel, table_index=idx, out_form=1)
        assert got1.shape == (B, 2, P * N + 1) and np.array_equal(got1, want_ext), ("out_form 1", idx)
        got2 = eng.mk_cmux_net(data, net, sel, table_index=idx, out_form=2)
        assert eng.last_timing_ms(1) > 0 and got2.shape == (B, 2, P * s.n + 1)
        assert np.array_equal(got2, want_ks), ("out_form 2", idx)
    s.ck.close()


# ---- 3. GPU: a tree-shaped network is the multi-key CMUX tree ----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("P,N,l,beta", [(2, 64, 3, 7), (3, 32, 2, 8)])
def test_gpu_mk_tree_net_equals_mk_cmux_tree(tfhe, orc, P, N, l, beta):
    """Word for word in every form and at every depth, also where the set is not exact for arbitrary words: the two kernels make the
    same floating-point operations in the same order."""
    from tfhe_jl_amd import leveled
    B, T = 3, 2
    owners = list(range(P)) + [P - 1, 0]
    s = Setup(tfhe, P, N, l, beta, 6400 + P + N, owners)
    eng = s.ck.engine(0)
    full = s.encrypt(_words(s.rng, T * 8, N)).reshape(T, 8, P + 1, N)
    arbitrary = _words(s.rng, T, 8, P + 1, N)
    arbitrary[0, 1], arbitrary[1, 2] = 2**31 - 1, -2**31
    index = np.array([1, 0, 1], np.int32)
    eng.mk_tgsw_load(s.tgsw, s.owners)
    for depth in (1, 2, 3):
        net = leveled.tree_net(depth)
        sel = s.rng.integers(0, len(owners), (B, depth)).astype(np.int32)
        sel[0, :] = [v % P for v in range(depth)]
        for tables in (full, arbitrary):
            data = np.ascontiguousarray(tables[:, :1 << depth])
            for form in (0, 1, 2):
                tree = eng.mk_cmux_tree(data, sel, table_index=index, out_form=form)
                got = eng.mk_cmux_net(data, net, sel, table_index=index, out_form=form)
                assert got.shape == (B, 1) + tree.shape[1:] and np.array_equal(got[:, 0], tree), (depth, form)
        ref = s.tree(orc)                                                # ... and both are the schoolbook's words, not each other's mistake
        data = np.ascontiguousarray(full[:, :1 << depth])
        assert np.array_equal(eng.mk_cmux_net(data, net, sel[:1], table_index=index[:1], out_form=0)[0, 0], ref.tree(data[1], sel[0]).astype(np.int32))
    s.ck.close()


# ---- 4. GPU: spectrum accumulators in global memory --------------------------------------------------------------------------------
COPY_NET = ([2, 1], [[0, 1, 0], [2, 2, 1], [1, 0, 1]])                    # two levels, a copy node at level 0, src0 > src1 at level 1


@pytest.mark.gpu
def test_gpu_mk_accumulators_in_global_memory_small(tfhe, orc):
    from tfhe_jl_amd import leveled
    P, N, l, beta = 2, 64, 3, 7
    s = Setup(tfhe, P, N, l, beta, 6600, owners=[1, 0, 1])
    eng = s.ck.engine(0)
    data = s.encrypt(_words(s.rng, 3, N))
    net = leveled.CmuxNet(*COPY_NET, entries=3, variables=2)
    sel = np.array([[0, 1], [2, 0]], np.int32)
    eng.mk_tgsw_load(s.tgsw, s.owners)
    lds = [eng.mk_cmux_net(data, net, sel, out_form=f) for f in (0, 1, 2)]
    assert eng.last_kernel_name() == f"mk_cmux_net_level_kernel(N={N},P={P},l={l})"
    eng.set_option("anyn_spec", 1)
    glob = [eng.mk_cmux_net(data, net, sel, out_form=f) for f in (0, 1, 2)]
    assert eng.last_kernel_name() == f"mk_cmux_net_level_kernel(N={N},P={P},l={l},spec=global)"
    for a, b in zip(lds, glob):
        assert np.array_equal(a, b)
    want, want_ext, want_ks = ref_rows(s.tree(orc, with_ks=True), net, data[None], [0, 0], sel, with_ks=True)
    assert np.array_equal(glob[0], want) and np.array_equal(glob[1], want_ext) and np.array_equal(glob[2], want_ks)
    s.ck.close()


@pytest.mark.gpu
def test_gpu_mk_accumulators_in_global_memory_n4096(tfhe, orc):
    """N = 4096 is the smallest degree at which buf + 3 accumulators + tmp pass 160 KB of LDS (tests/test_mk_leveled.py): the
    accumulators can only live in global memory; one row, against the schoolbook."""
    from tfhe_jl_amd import leveled
    P, N, l, beta = 2, 4096, 2, 6
    s = Setup(tfhe, P, N, l, beta, 6700, owners=[1, 0], n=2)
    eng = s.ck.engine(0)
    data = s.encrypt(_words(s.rng, 3, N))
    net = leveled.CmuxNet(*COPY_NET, entries=3, variables=2)
    sel = np.array([[1, 0]], np.int32)
    eng.mk_tgsw_load(s.tgsw, s.owners)
    got = eng.mk_cmux_net(data, net, sel, out_form=0)
    assert eng.last_kernel_name() == f"mk_cmux_net_level_kernel(N={N},P={P},l={l},spec=global)"
    want, _, _ = ref_rows(s.tree(orc), net, data[None], [0], sel)
    assert np.array_equal(got, want)
    s.ck.close()


# ---- 5. GPU: workspaces sized by every level, regrown correctly, shared with the tree ------------------------------------------------
@pytest.mark.gpu
def test_gpu_mk_workspace_parity_and_regrowth(tfhe, orc):
    """Widths [2, 6, 3, 7, 1] as the first call of a fresh context (the odd levels are wider than level 0 and than every even level:
    buffers sized by level 0, or both by one maximum taken over the wrong parity, overflow or misplace rows), then a one-node network,
    then the first again, then a CMUX tree on the same context and buffers."""
    from tfhe_jl_amd import leveled
    P, N, l, beta, B, E, V = 2, 64, 3, 7, 2, 4, 5
    s = Setup(tfhe, P, N, l, beta, 6500, owners=[0, 1, 1, 0, 1])
    eng = s.ck.engine(0)
    data = s.encrypt(_words(s.rng, E, N)).reshape(1, E, P + 1, N)
    widths = [2, 6, 3, 7, 1]
    nodes = []
    for v, w in enumerate(widths):
        below = E if v == 0 else widths[v - 1]
        nodes += [[i % below, (i + 1 + v) % below if below > 1 else 0, (i + v) % V] for i in range(w)]
    big = leveled.CmuxNet(widths, nodes, entries=E, variables=V)
    one = leveled.CmuxNet([1], [[2, 0, 4]], entries=E, variables=V)
    sel = np.array([[0, 1, 2, 3, 4], [4, 2, 0, 1, 3]], np.int32)
    ref = s.tree(orc)
    eng.mk_tgsw_load(s.tgsw, s.owners)
    for net in (big, one, big):
        want, want_ext, _ = ref_rows(ref, net, data, [0] * B, sel)
        assert np.array_equal(eng.mk_cmux_net(data, net, sel, out_form=0), want), list(net.widths)
        assert np.array_equal(eng.mk_cmux_net(data, net, sel, out_form=1), want_ext), list(net.widths)
    tree = np.stack([ref.tree(data[0], sel[g, :2]) for g in range(B)])
    assert np.array_equal(eng.mk_cmux_tree(data, sel[:, :2], out_form=0), tree.astype(np.int32))
    want, _, _ = ref_rows(ref, big, data, [0] * B, sel)
    assert np.array_equal(eng.mk_cmux_net(data, big, sel, out_form=0), want)
    s.ck.close()


# ---- 6. GPU: the millionaires' problem at full size ----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_mk_less_than_16_bits_full_size_two_parties(tfhe, orc):
    """mktfhe_parameters_2party, less_than_net(16), B = 8: party 0 uni-encrypts the bits of x, party 1 those of y, the 256 selectors are
    expanded on the device, out_form 2: mk_decrypt returns x < y for all 8; row 0 at out_form 1 with the host expansion equals the
    extraction of the schoolbook network word for word."""
    from tfhe_jl_amd import leveled
    p = tfhe.mktfhe_parameters_2party
    N, l, beta, P, d = p.tlwe_polynomial_degree, p.bs_decomp_length, p.bs_log2_base, 2, 16
    rng = np.random.default_rng(8816)
    sks = [tfhe.SecretKey(rng, p) for _ in range(P)]
    shared = tfhe.SharedKey(rng, p)
    parts = [tfhe.CloudKeyPart(rng, sk, shared, keep_tlwe_key=True) for sk in sks]
    ck = tfhe.MKCloudKey(parts, expand="device")
    net, table = leveled.less_than_net(d)
    assert net.levels == 32 and net.widths.max() == 4 and net.products == 48
    pairs = [(12345, 12345), (40000, 40001), (40001, 40000), (0, 65535), (65535, 0), (0x8000, 0x7FFF)]
    pairs += [tuple(int(v) for v in rng.integers(0, 65536, 2)) for _ in range(2)]
    bits = np.array([_compare_bits(x, y, d) for x, y in pairs])
    owners = np.array([0] * d + [1] * d, np.int32)                       # variables 0 ... 15: x, party 0; 16 ... 31: y, party 1
    uni = [np.zeros((8, 2 * d, l, N), np.int32) for _ in range(6)]
    for i in range(P):
        cols = np.nonzero(owners == i)[0]
        arrs = leveled.mk_tgsw_uni_encrypt_bits(rng, parts[i].tlwe_key, shared, parts[i].public_b, bits[:, cols].reshape(-1))
        for dst, a in zip(uni, arrs):
            dst[:, cols] = a.reshape(8, cols.size, l, N)
    data = leveled.table_to_tlwe(table, N, k=P)
    out = leveled.mk_cmux_net_lookup(ck, data, net, uni, owners)
    assert out.shape == (8, P * p.lwe_size + 1)
    assert ck.engine(0).last_kernel_name() == f"mk_cmux_net_level_kernel(N={N},P={P},l={l})"
    assert np.array_equal(tfhe.mk_decrypt(sks, out), np.array([x < y for x, y in pairs]))
    pub = np.stack([part.public_b for part in parts])
    tg = np.zeros((2 * d, 2 * l * P + 2 * l, N), np.int32)
    for v in range(2 * d):
        tg[v] = leveled.mk_tgsw_expand(p, pub, owners[v], *[a[0, v:v + 1] for a in uni])[0]
    ref = MKTree(orc, N, l, beta, P, tg, owners)
    ext = leveled.mk_cmux_net_lookup(ck, data, net, [a[:1] for a in uni], owners, out_form=1, expand="host")
    assert ext.shape == (1, 1, P * N + 1)
    assert np.array_equal(ext[0, 0], ref.extract(mk_net_ref(ref, net, data, range(2 * d))[0]).astype(np.int32))
    ck.close()


# ---- 7. GPU: the contract ----------------------------------------------------------------------------------------------------------
class _Call:
    """A valid raw call of tfhe_mk_cmux_net_batch whose arguments can be replaced one at a time."""

    def __init__(self, eng, data, net, sel):
        self.eng, self.F = eng, int(net.widths[-1])
        self.base = dict(data=data, T=data.shape[0], E=data.shape[1], table_index=None, widths=net.widths, levels=net.levels, nodes=net.nodes,
                         sel=sel, V=sel.shape[1], B=sel.shape[0], out_form=0)

    def __call__(self, eng=None, **over):
        eng = eng or self.eng
        a = dict(self.base, **over)
        out = np.zeros((self.base["B"], self.F) + self.base["data"].shape[2:], np.int32)
        rc = eng._lib.tfhe_mk_cmux_net_batch(eng._h, _ptr(a["data"]), a["T"], a["E"], _ptr(a["table_index"]), _ptr(a["widths"]), a["levels"],
                                             _ptr(a["nodes"]), _ptr(a["sel"]), a["V"], _ptr(out), a["B"], a["out_form"])
        return rc, eng._lib.tfhe_last_error(eng._h).decode(), out


@pytest.mark.gpu
def test_gpu_mk_contract_refusals_leave_the_context_usable(tfhe, orc):
    from tfhe_jl_amd import leveled
    P, N, l, beta, E, V, S = 2, 64, 3, 7, 3, 2, 3
    s = Setup(tfhe, P, N, l, beta, 9700, owners=[0, 1, 0])
    eng = s.ck.engine(0)
    data = s.encrypt(_words(s.rng, E, N))[None]
    net = leveled.CmuxNet(*COPY_NET, entries=E, variables=V)
    sel = np.array([[0, 1], [2, 0]], np.int32)
    want, want_ext, want_ks = ref_rows(s.tree(orc, with_ks=True), net, data, [0, 0], sel, with_ks=True)
    call = _Call(eng, data, net, sel)
    xs, ys = tfhe.mk_encrypt(s.rng, s.sks, [True, False, True]), tfhe.mk_encrypt(s.rng, s.sks, [True, True, False])

    def nand_works(e):
        assert np.array_equal(tfhe.mk_decrypt(s.sks, e.mk_gate_nand(xs, ys)), [False, True, True])

    def still_right():
        rc, msg, out = call()
        assert rc == 0 and np.array_equal(out, want), msg

    def refused(code, word, **over):
        rc, msg, _ = call(**over)
        assert rc == code and word in msg and "mk_cmux_net_batch" in msg, (over.keys(), rc, msg)
        still_right()

    rc, msg, _ = call()
    assert rc == NO_KEY and "selector" in msg                          # no selector set yet
    nand_works(eng)
    eng.mk_tgsw_load(s.tgsw, s.owners)
    still_right()
    for name in ("data", "widths", "nodes", "sel"):
        refused(INVALID, "NULL", **{name: None})
    refused(INVALID, "negative", B=-1)
    for levels in (0, -1, 1025, 4096):
        refused(INVALID, "levels", levels=levels)
    for w in (0, 4097, -3):
        refused(INVALID, "widths[1]", widths=np.array([2, w], np.int32))
    refused(INVALID, "E =", E=0)
    refused(INVALID, "V =", V=0)
    refused(INVALID, "T =", T=0)
    bad = net.nodes.copy(); bad[1, 0] = 3                              # level 0: a source past the table
    refused(INVALID, "node 1 of level 0: src0 = 3", nodes=bad)
    bad = net.nodes.copy(); bad[2, 1] = 2                              # level 1: a source past the two nodes below
    refused(INVALID, "node 0 of level 1: src1 = 2", nodes=bad)
    bad = net.nodes.copy(); bad[0, 0] = -1
    refused(INVALID, "src0 = -1", nodes=bad)
    for var in (V, -1):
        bad = net.nodes.copy(); bad[2, 2] = var
        refused(INVALID, f"var = {var}", nodes=bad)
    for sidx in (S, -1):
        bad = sel.copy(); bad[1, 0] = sidx
        refused(INVALID, "sel[1][0]", sel=bad)
    for t in (1, -1):
        refused(INVALID, "table_index[1]", table_index=np.array([0, t], np.int32))
    for form in (3, -1):
        refused(INVALID, "out_form", out_form=form)
    refused(INVALID, "exceed one launch", B=2**30)                     # B * widths[0] = 2^31 (refused before sel is read)
    rc, msg, _ = call(B=0, data=None, sel=None)
    assert rc == 0
    eng.set_option("measure_margin", 1)
    rc, msg, _ = call()
    assert rc == STATE and "measure_margin" in msg
    eng.set_option("measure_margin", 0)
    still_right()
    assert np.array_equal(eng.mk_cmux_net(data, net, sel, out_form=1), want_ext) and np.array_equal(eng.mk_cmux_net(data, net, sel), want_ks)
    # no multi-key bootstrapping key, then no selector set, then out_form 2 without the multi-key keyswitch key; forms 0 and 1 do not need it
    raw = tfhe.Engine(s.p)
    rc, msg, _ = call(raw)
    assert rc == NO_KEY and "bootstrapping key" in msg
    raw.mk_load_bootstrap_key(s.ck.bootstrap_key, P)
    rc, msg, _ = call(raw)
    assert rc == NO_KEY and "selector" in msg
    raw.mk_tgsw_load(s.tgsw, s.owners)
    rc, msg, _ = call(raw, out_form=2)
    assert rc == NO_KEY and "keyswitch" in msg
    assert np.array_equal(raw.mk_cmux_net(data, net, sel, out_form=1), want_ext)
    raw.mk_load_keyswitch_key(s.ck.keyswitch_key, P)
    assert np.array_equal(raw.mk_cmux_net(data, net, sel), want_ks)
    raw.close()
    # a single-key context: the new call is refused, its own network call and its gates go on
    p1 = tfhe.SchemeParameters(16, 1 / 2**15, N, 1, l, beta, 1e-7, 8, 2, 1 / 2**15, 1)
    sk1, ck1 = tfhe.make_key_pair(s.rng, p1)
    e1 = ck1.engine(0)
    rc, msg, _ = call(e1)
    assert rc == STATE and "single-key" in msg
    bx = tfhe.encrypt(s.rng, sk1, [True, False]).data
    assert np.array_equal(tfhe.decrypt(sk1, e1.gates(np.zeros(2, np.uint8), bx, bx)), [False, True])
    ck1.close()
    # a multi-device context
    multi = s.ck.engine([0, 0])
    rc, msg, _ = call(multi)
    assert rc == STATE and "multi-device" in msg
    nand_works(multi)
    # an injected allocation failure through the new entry point: NOMEM, and the context goes on working
    lib = eng._lib
    assert lib.tfhe_set_option(None, b"debug_fail_alloc_after", 1) == 0
    rc, msg, _ = call()
    lib.tfhe_set_option(None, b"debug_fail_alloc_after", 0)
    assert rc == NOMEM and "memory" in msg, (rc, msg)
    still_right()
    nand_works(eng)
    s.ck.close()


@pytest.mark.gpu
def test_gpu_mk_oversized_network_is_refused_before_allocating(tfhe):
    """1024 levels of 4096 nodes at B = 2^19 - 1 rows: one workspace alone is 1.6 TB.  TFHE_ERR_NOMEM, computed and refused before any
    allocation (hipMemGetInfo reads unchanged), and the context goes on working."""
    from tfhe_jl_amd import leveled
    P, N, l, beta = 2, 64, 3, 7
    s = Setup(tfhe, P, N, l, beta, 9800, owners=[1], bits=[1])
    eng = s.ck.engine(0)
    eng.mk_tgsw_load(s.tgsw, s.owners)
    table = _gate_table([True, False], N, P)
    small = leveled.CmuxNet([1], [[1, 0, 0]])                         # selector bit 1 picks src1 = entry 0
    assert list(tfhe.mk_decrypt(s.sks, eng.mk_cmux_net(table, small, np.zeros((1, 1), np.int32))[:, 0])) == [True]
    B = 2**19 - 1
    huge = leveled.CmuxNet([4096] * 1024, np.zeros((4096 * 1024, 3), np.int32), entries=2, variables=1)
    sel = np.zeros((B, 1), np.int32)
    before = _mem_free()
    rc = eng._lib.tfhe_mk_cmux_net_batch(eng._h, _ptr(table), 1, 2, None, _ptr(huge.widths), huge.levels, _ptr(huge.nodes), _ptr(sel), 1,
                                         _ptr(np.zeros(1, np.int32)), B, 0)
    assert rc == NOMEM and "MB" in eng._lib.tfhe_last_error(eng._h).decode()
    assert _mem_free() == before
    assert list(tfhe.mk_decrypt(s.sks, eng.mk_cmux_net(table, small, np.zeros((1, 1), np.int32))[:, 0])) == [True]
    s.ck.close()
