"""Leveled mode: external products and CMUX trees on the caller's own TLWE / TGSW samples, no blind rotation.

A table of 2^d TLWE samples is folded by d levels of CMUXes d0 + C (.) (d1 - d0) (the form of bootstrap.jl:19-23, with
tgsw_extern_mul, tgsw.jl:125-129), level v selecting by the TGSW encryption C of address bit v (bit 0 = the lowest): what is
left is table[address], at 2^d - 1 external products.  Each level adds the noise of one external product (about
sqrt((k+1) l N) 2^(beta-1) bs_noise_stddev plus the gadget truncation 2^-(l beta + 1) (1 + k N / 2)^(1/2): 3e-4 of the torus per
level at tfhe_parameters_80) to a message window of 1/8, so d = 8 is far inside it; extracted at coefficient 0 and keyswitched
(out_form 2) the result is an LWE sample under the gate key and an operand of any gate_* / Circuit.

The host side mirrors the reference's constructors under the TLWE key that CloudKey draws and now keeps as
`secret_key.tlwe_key`: tlwe_encrypt (tlwe.jl:63-73 plus a message on the body), tgsw_encrypt_bits (tgsw.jl:84-88 at
bs_noise_stddev).  The device side is Engine.tgsw_load / extern_mul / cmux_tree (tfhe_tgsw_load, tfhe_extern_mul_batch,
tfhe_cmux_tree_batch); cmux_lookup strings them together.

A CMUX network (CmuxNet; Engine.cmux_net, tfhe_cmux_net_batch; cmux_net_lookup) is the same CMUX wired by a public netlist instead of
by halving: the TFHE paper's evaluation of a deterministic automaton or an ordered decision diagram on TGSW-encrypted letters.  A
function of d encrypted bits with a small automaton then costs a few CMUXes per bit instead of 2^d - 1 per lookup: dfa_net builds the
network of an automaton, less_than_net the five-state comparator of two d-bit integers, tree_net the network of cmux_lookup.

Under a multi-key cloud key (the mk_* functions below) the selectors are jointly encrypted: each party uni-encrypts the address bits
it owns (mk_tgsw_uni_encrypt_bits: RGSW.UniEnc, mk_internals.jl:185-227) under the TLWE key that CloudKeyPart(..., keep_tlwe_key=True)
keeps, the cloud expands them against all public keys (mk_tgsw_expand: RGSW.Expand, :304-345; or on the device) and folds a table of
MK TLWE samples [P+1][N] with mk_tgsw_extern_mul (:348-391).  Keyswitched (out_form 2) the result is a multi-key LWE sample that
mk_decrypt and every mk_gate accept.  Engine.mk_tgsw_load / mk_tgsw_expand_load / mk_extern_mul / mk_cmux_tree; mk_cmux_lookup strings
them together.  The CMUX networks above run on the same selectors (Engine.mk_cmux_net, tfhe_mk_cmux_net_batch; mk_cmux_net_lookup):
the comparison of two integers that two parties hold is less_than_net on their uni-encrypted bits.

A network with monomial edges (RotNet; Engine.rot_net, tfhe_rot_net_batch; rot_net_lookup) multiplies each source of a CMUX by a public
X^rot (mul_by_monomial, bootstrap.jl:21, :54).  CMUX(C_b; acc, X^(-2^b) acc) for the low address bits b is the blind rotation by TGSW
bits: a table packed N entries to a sample (pack_table_to_tlwe, "vertical packing") is read at 2^(d - log2 N) - 1 + log2 N external
products instead of 2^d - 1 (packed_lookup_net, packed_lookup), and an automaton with X^weight on its transitions (wfa_net) returns
X^(sum of weights) table[end state]: f(popcount(x)) of up to N - 1 encrypted bits is one state and one product per bit.  Entries of
w bits are packed N / w to a sample and leave as w outputs of one address walk (pack_words_to_tlwe, packed_words_net).  The same
networks run on jointly encrypted variables under a multi-key cloud key (Engine.mk_rot_net, tfhe_mk_rot_net_batch; mk_rot_net_lookup,
mk_packed_lookup): a table packed N entries to an MK TLWE sample is read at an address whose bits several parties own.

The blind rotation of the caller's accumulators (Engine.blind_rotate, tfhe_blind_rotate_batch; blind_rotate_lookup) is the way back from
the bootstrapped half: the bootstrapping key, loaded as a selector set (bootstrap_key_selectors), rotates a TLWE sample the caller
supplies by an LWE sample that gates or lookups computed.  An encrypted test polynomial (private_lut_encrypt) is a lookup table the
server evaluates without reading it; the output of a CMUX tree over TGSW address bits, rotated by an LWE digit, is a table of p 2^d
entries addressed in part by a computed value (two_stage_lookup); and with out_form 0 a bootstrap's result leaves as a TLWE sample, an
entry of the tables cmux_lookup / cmux_net_lookup read (pbs_to_tlwe).  The accumulator's own noise passes through unrefreshed; the
rotation adds what a bootstrap's rotation adds.

Under a multi-key cloud key the same bridge is Engine.mk_blind_rotate (tfhe_mk_blind_rotate_batch; mk_blind_rotate_lookup): the multi-key
bootstrapping key is a selector set of P n expanded RGSW samples, party-major (mk_bootstrap_key_selectors), and rotates an MK TLWE
sample by a multi-key LWE sample as it lies in memory.  mk_private_lut_encrypt is one party's private function on jointly encrypted
data, mk_two_stage_lookup a table of p 2^d entries addressed by jointly encrypted TGSW bits and a computed digit, mk_pbs_to_tlwe a
multi-key bootstrap's result as an entry of the tables mk_cmux_lookup / mk_cmux_net_lookup read.

mk_two_stage_lookup_device is mk_two_stage_lookup's program between the device-resident tables of a multi-key engine (the MK TLWE table
of Engine.mk_tlwe_alloc and the multi-key wire table): the key's selectors are loaded once, a request's address bits are swapped
behind them (Engine.mk_tgsw_expand_update), the tree writes slots (Engine.mk_rot_net_level) and the rotation reads its digit from a wire
and writes wires (Engine.mk_blind_rotate_level).
"""
import numpy as np

from . import mk_keys
from .keys import _tlwe_encrypt_zero_many, make_bootstrap_key
from .lut import make_test_vector
from .lwe import LweKey, LweSampleArray
from .numeric import dtot32, negacyclic_mul_binary, rand_uniform_torus32, wrap32


def _tlwe_key(secret_key):
    key = getattr(secret_key, "tlwe_key", None)
    if key is None:
        raise ValueError("this SecretKey has no tlwe_key yet: CloudKey(rng, secret_key) draws it and keeps it there")
    return key


def tlwe_trivial(polys, k=1):
    """tlwe_noiseless_trivial (tlwe.jl:77-81) of each message polynomial: int32 [..., N] -> int32 [count][k+1][N], zero masks."""
    mu = np.atleast_2d(np.asarray(polys, np.int32))
    out = np.zeros((mu.shape[0], k + 1, mu.shape[1]), np.int32)
    out[:, k, :] = mu
    return out


def tlwe_encrypt(rng, secret_key, polys):
    """tlwe_encrypt_zero (tlwe.jl:63-73) at bs_noise_stddev plus the message polynomial on the body: int32 [..., N] Torus32
    messages -> int32 [count][k+1][N] under secret_key.tlwe_key."""
    key = _tlwe_key(secret_key)
    mu = np.atleast_2d(np.asarray(polys, np.int32))
    if mu.shape[1] != key.N:
        raise ValueError(f"message polynomials must have {key.N} coefficients, got {mu.shape[1]}")
    out = _tlwe_encrypt_zero_many(rng, secret_key.params.bs_noise_stddev, key, mu.shape[0]).astype(np.int32)
    out[:, key.k, :] = wrap32(out[:, key.k, :].astype(np.int64) + mu)
    return out


def tlwe_phase(secret_key, samples):
    """body - sum_c a_c (*) key_c (negacyclic) of TLWE samples int32 [count][k+1][N]: the noisy message polynomials [count][N]."""
    key = _tlwe_key(secret_key)
    s = np.asarray(samples, np.int32)
    if s.ndim == 2:
        s = s[None]
    ph = s[:, key.k, :].astype(np.int64)
    for c in range(key.k):
        ph = ph - negacyclic_mul_binary(key.key[c], s[:, c, :]).astype(np.int64)
    return wrap32(ph)


def tgsw_encrypt_bits(rng, secret_key, bits):
    """tgsw_encrypt (tgsw.jl:84-88) of each bit at bs_noise_stddev under secret_key.tlwe_key, in the flat layout the engine takes:
    int32 [S][l][k+1][k+1][N] = samples[p, j].a[c] — S entries of the bootstrapping key's canonical form (bootstrap.jl:6-15 makes
    exactly these of the LWE key's bits)."""
    key = _tlwe_key(secret_key)
    p = secret_key.params
    b = np.asarray(bits).astype(bool).reshape(-1).astype(np.int32)
    return make_bootstrap_key(rng, p.bs_noise_stddev, LweKey(None, b.size, key=b), key, p.bs_decomp_length, p.bs_log2_base)


def encode_gate_bit(value):
    """A table entry as the gate encoding of a bit: +1/8 for true, -1/8 for false (gates.jl)."""
    return (1 << 29) if value else -(1 << 29)


def table_to_tlwe(values, N, k=1, encode=encode_gate_bit, rng=None, secret_key=None):
    """A table as TLWE samples int32 [len(values)][k+1][N]: entry i carries encode(values[i]) (a Torus32 word) on coefficient 0 of
    its message polynomial, which is where tlwe_extract_sample (tlwe.jl:55-59) reads.  Trivial (noiseless, public) samples, or —
    with rng and secret_key — encryptions under secret_key.tlwe_key (a private table)."""
    mu = np.zeros((len(values), N), np.int32)
    mu[:, 0] = wrap32(np.array([int(encode(v)) for v in values], np.int64))
    if secret_key is None:
        return tlwe_trivial(mu, k)
    if rng is None:
        raise ValueError("an encrypted table needs rng as well as secret_key")
    return tlwe_encrypt(rng, secret_key, mu)


def cmux_lookup(ck, tables, address_tgsw, out_form=2, device=0, table_index=None):
    """table[address] for B encrypted addresses.  tables: int32 [2^d][k+1][N] (table_to_tlwe) or [T][2^d][k+1][N] with table_index
    [B]; address_tgsw: int32 [B][d][l][k+1][k+1][N], bit v of address g encrypted by tgsw_encrypt_bits (bit 0 = the lowest).
    out_form 2 (default): an LweSampleArray under the gate key, ready for gate_* / Circuit; 1: the extracted samples int32
    [B][k N + 1]; 0: the TLWE samples int32 [B][k+1][N]."""
    a = np.asarray(address_tgsw, np.int32)
    if a.ndim != 6:
        raise ValueError(f"address_tgsw must be [B][depth][l][k+1][k+1][N], got {a.shape}")
    B, depth = a.shape[:2]
    eng = ck.engine(device)
    eng.tgsw_load(a.reshape((B * depth,) + a.shape[2:]))
    sel = np.arange(B * depth, dtype=np.int32).reshape(B, depth)
    out = eng.cmux_tree(tables, sel, table_index=table_index, out_form=out_form)
    return LweSampleArray(out) if out_form == 2 else out


# ---- CMUX networks: automata and decision diagrams ------------------------------------------------------------------------------
NET_MAX_LEVELS, NET_MAX_WIDTH = 1024, 4096


def _check_netlist(widths, nodes, fields, entries, variables, two_n):
    """The validation of net_check_netlist / rot_check_netlist (csrc/leveled_checks.hpp) with their messages: widths, then every record's
    sources against the level below, its var against V and, in a five-word record, its rotations against [0, two_n).  Returns widths
    and nodes as int32 arrays, E and V."""
    w = np.asarray(widths)
    if w.ndim != 1 or not np.issubdtype(w.dtype, np.integer) or not 1 <= w.size <= NET_MAX_LEVELS:
        raise ValueError(f"widths must be 1 ... {NET_MAX_LEVELS} integers, got shape {w.shape}")
    for v, x in enumerate(w):
        if not 1 <= x <= NET_MAX_WIDTH:
            raise ValueError(f"widths[{v}] = {x} (1 ... {NET_MAX_WIDTH})")
    nd = np.asarray(nodes)
    if not np.issubdtype(nd.dtype, np.integer) or nd.shape != (int(w.sum()), len(fields)):
        raise ValueError(f"nodes must be integers [{int(w.sum())}][{len(fields)}] = ({', '.join(fields)}), got {nd.shape}")
    nd = nd.astype(np.int64)
    need_e = int(nd[:w[0], :2].max()) + 1
    need_v = int(nd[:, 2].max()) + 1
    E = need_e if entries is None else int(entries)
    V = need_v if variables is None else int(variables)
    if E < 1 or V < 1:
        raise ValueError(f"entries = {E}, variables = {V} (at least one each)")
    first = 0
    for v, x in enumerate(w):
        below = E if v == 0 else int(w[v - 1])
        lv = nd[first:first + int(x)]
        bad = np.argwhere((lv[:, :2] < 0) | (lv[:, :2] >= below))
        if bad.size:
            i, e = (int(t) for t in bad[0])
            what = "table entries" if v == 0 else "nodes"
            raise ValueError(f"node {i} of level {v}: src{e} = {lv[i, e]} is outside the {below} {what} below")
        bad = np.flatnonzero((lv[:, 2] < 0) | (lv[:, 2] >= V))
        if bad.size:
            raise ValueError(f"node {bad[0]} of level {v}: var = {lv[bad[0], 2]} is outside [0, {V})")
        bad = np.argwhere((lv[:, 3:] < 0) | (lv[:, 3:] >= two_n))
        if bad.size:
            i, e = (int(t) for t in bad[0])
            raise ValueError(f"node {i} of level {v}: {fields[3 + e]} = {lv[i, 3 + e]} is outside [0, {two_n})")
        first += int(x)
    return np.ascontiguousarray(w, np.int32), np.ascontiguousarray(nd, np.int32), E, V


class CmuxNet:
    """The public wiring of a CMUX network, validated as tfhe_cmux_net_batch validates it.  widths: the node count of each level (1 ...
    1024 levels of 1 ... 4096 nodes); nodes: int32 [sum widths][3] = (src0, src1, var) in level order.  Node i of level v is
    in[src0] + C_var (.) (in[src1] - in[src0]) — a variable that is 1 picks src1 — with `in` the table entries for v = 0 and the outputs
    of level v - 1 above; src0 == src1 is a copy.  The outputs are the nodes of the last level.  `entries` (the table length E) and
    `variables` (V) default to the smallest counts the nodes need; given, the nodes are checked against them."""

    def __init__(self, widths, nodes, entries=None, variables=None):
        self.widths, self.nodes, self.entries, self.variables = _check_netlist(widths, nodes, ("src0", "src1", "var"), entries, variables, 0)
        self.levels = int(self.widths.size)

    def level(self, v):
        """The records of level v, int32 [widths[v]][3]."""
        first = int(self.widths[:v].sum())
        return self.nodes[first:first + int(self.widths[v])]

    @property
    def products(self):
        """External products per row: the nodes that are not copies."""
        return int(np.count_nonzero(self.nodes[:, 0] != self.nodes[:, 1]))

    def evaluate_clear(self, entries, bits):
        """The same wiring on plain values: the outputs of the last level for table `entries` and variable values `bits`."""
        cur = list(entries)
        if len(cur) < self.entries or len(bits) < self.variables:
            raise ValueError(f"the network reads {self.entries} entries and {self.variables} variables, got {len(cur)} and {len(bits)}")
        for v in range(self.levels):
            cur = [cur[s1] if bits[var] else cur[s0] for s0, s1, var in self.level(v).tolist()]
        return cur


def tree_net(depth):
    """The network of cmux_lookup / Engine.cmux_tree: 2^depth entries, level v folds the pairs (2i, 2i + 1) by variable v."""
    if not 1 <= depth <= 12:
        raise ValueError(f"depth = {depth} (1 ... 12)")
    widths = [1 << (depth - 1 - v) for v in range(depth)]
    nodes = [(2 * i, 2 * i + 1, v) for v in range(depth) for i in range(widths[v])]
    return CmuxNet(widths, nodes, entries=1 << depth, variables=depth)


def dfa_net(delta0, delta1, start, steps, letter_var=None):
    """The backward evaluation of a deterministic automaton (the TFHE paper's leveled automaton evaluation).  State q moves to delta0[q]
    on letter 0 and to delta1[q] on letter 1; the automaton reads `steps` letters from `start`, letter j being variable letter_var[j]
    (default: j).  Level v handles letter steps - 1 - v and has one node per state reachable after that many letters, in increasing
    state order; a state whose two transitions agree (an absorbing state) becomes a copy node.  Level 0 reads table entry q = the weight
    of ending in state q (E = number of states); the one output is the weight of the state the letters lead to."""
    d0, d1 = [int(q) for q in delta0], [int(q) for q in delta1]
    Q = len(d0)
    if Q < 1 or len(d1) != Q or any(not 0 <= q < Q for q in d0 + d1) or not 0 <= start < Q:
        raise ValueError("delta0 and delta1 must map every state to a state, and start must be a state")
    if not 1 <= steps <= NET_MAX_LEVELS:
        raise ValueError(f"steps = {steps} (1 ... {NET_MAX_LEVELS})")
    var = list(range(steps)) if letter_var is None else [int(x) for x in letter_var]
    if len(var) != steps:
        raise ValueError(f"letter_var must name a variable for each of the {steps} letters")
    reach = [[int(start)]]                                           # reach[j]: the states after j letters, sorted
    for j in range(steps - 1):
        reach.append(sorted({d[q] for q in reach[-1] for d in (d0, d1)}))
    widths, nodes = [], []
    for v in range(steps):
        j = steps - 1 - v
        place = {q: q for q in range(Q)} if v == 0 else {q: i for i, q in enumerate(reach[j + 1])}
        widths.append(len(reach[j]))
        nodes += [(place[d0[q]], place[d1[q]], var[j]) for q in reach[j]]
    return CmuxNet(widths, nodes, entries=Q, variables=max(var) + 1)


def less_than_net(bits):
    """x < y for two `bits`-bit unsigned integers as a five-state automaton over the letters x_{d-1}, y_{d-1}, ..., x_0, y_0 (highest
    bit first): equal so far (0), equal and x's bit was 0 (1) or 1 (2), x < y decided (3), x > y decided (4).  Returns (net, table):
    the network over variables x_0 ... x_{d-1}, y_0 ... y_{d-1} (variable b = bit b of x, d + b = bit b of y; 2 d levels of at most 4
    nodes) and its end-state table, the truth of x < y in each of the five states — table_to_tlwe(table, N, k) is the data."""
    d = int(bits)
    if not 1 <= d <= NET_MAX_LEVELS // 2:
        raise ValueError(f"bits = {bits} (1 ... {NET_MAX_LEVELS // 2})")
    letter_var = [(d - 1 - j // 2) + (d if j & 1 else 0) for j in range(2 * d)]
    net = dfa_net([1, 0, 4, 3, 4], [2, 3, 0, 3, 4], 0, 2 * d, letter_var)
    return net, [False, False, False, True, False]


def cmux_net_lookup(ck, data, net, bits_tgsw, out_form=2, device=0, table_index=None):
    """The network `net` on B rows of encrypted variables.  data: int32 [E][k+1][N] (table_to_tlwe) or [T][E][k+1][N] with table_index
    [B]; bits_tgsw: int32 [B][V][l][k+1][k+1][N], variable v of row g encrypted by tgsw_encrypt_bits.  out_form 2 (default): an
    LweSampleArray under the gate key, ready for gate_* / Circuit, of B F samples (row g's output i at g F + i; F = 1 for an
    automaton); 1: the extracted samples int32 [B][F][k N + 1]; 0: the TLWE samples int32 [B][F][k+1][N]."""
    a = np.asarray(bits_tgsw, np.int32)
    if a.ndim != 6:
        raise ValueError(f"bits_tgsw must be [B][V][l][k+1][k+1][N], got {a.shape}")
    B, V = a.shape[:2]
    eng = ck.engine(device)
    eng.tgsw_load(a.reshape((B * V,) + a.shape[2:]))
    sel = np.arange(B * V, dtype=np.int32).reshape(B, V)
    out = eng.cmux_net(data, net, sel, table_index=table_index, out_form=out_form)
    return LweSampleArray(out.reshape(-1, out.shape[-1])) if out_form == 2 else out


# ---- CMUX networks with monomial edges: packed tables and weighted automata ------------------------------------------------------
def _monomial_clear(p, r, N):
    """X^r p mod (X^N + 1) on a plain integer polynomial [N], 0 <= r < 2N: coefficient j moves to j + r mod 2N, the sign flips past N."""
    p = np.asarray(p)
    if r >= N:
        p, r = -p, r - N
    return np.concatenate([-p[N - r:], p[:N - r]])


class RotNet:
    """The public wiring of a CMUX network with monomial edges over polynomials of `degree` N coefficients, validated as
    tfhe_rot_net_batch validates it.  widths as CmuxNet's; nodes: int32 [sum widths][5] = (src0, src1, var, rot0, rot1) in level order,
    the rotations in [0, 2N).  Node i of level v is X^rot0 in[src0] + C_var (.) (X^rot1 in[src1] - X^rot0 in[src0]) — a variable that is
    1 picks X^rot1 in[src1].  src0 == src1 with rot0 == rot1 is a rotated copy; src0 == src1 with rot0 != rot1 is a true product, the
    step of a blind rotation.  `entries` and `variables` as CmuxNet's."""

    def __init__(self, widths, nodes, degree, entries=None, variables=None):
        N = int(degree)
        if N < 2 or N & (N - 1):
            raise ValueError(f"degree = {degree} (a power of two, at least 2)")
        self.degree = N
        self.widths, self.nodes, self.entries, self.variables = _check_netlist(widths, nodes, ("src0", "src1", "var", "rot0", "rot1"), entries,
                                                                               variables, 2 * N)
        self.levels = int(self.widths.size)

    def level(self, v):
        """The records of level v, int32 [widths[v]][5]."""
        first = int(self.widths[:v].sum())
        return self.nodes[first:first + int(self.widths[v])]

    @property
    def products(self):
        """External products per row: the nodes that are not rotated copies."""
        nd = self.nodes
        return int(np.count_nonzero((nd[:, 0] != nd[:, 1]) | (nd[:, 3] != nd[:, 4])))

    def evaluate_clear(self, entries, bits):
        """The same wiring on plain integer polynomials [N] with the same negacyclic rotation: the outputs of the last level for table
        `entries` and variable values `bits`."""
        cur = [np.asarray(e) for e in entries]
        if len(cur) < self.entries or len(bits) < self.variables or any(e.shape != (self.degree,) for e in cur):
            raise ValueError(f"the network reads {self.entries} polynomials of {self.degree} coefficients and {self.variables} variables")
        for v in range(self.levels):
            cur = [_monomial_clear(cur[s1], r1, self.degree) if bits[var] else _monomial_clear(cur[s0], r0, self.degree)
                   for s0, s1, var, r0, r1 in self.level(v).tolist()]
        return cur


def _packing(count, N):
    """depth and r = min(depth, log2 N) of a packed table of `count` = 2^depth entries."""
    depth = int(count).bit_length() - 1
    if count < 2 or count != 1 << depth:
        raise ValueError(f"a packed table has 2^depth entries (depth >= 1), got {count}")
    return depth, min(depth, int(N).bit_length() - 1)


def pack_table_to_tlwe(values, N, k=1, encode=encode_gate_bit, rng=None, secret_key=None):
    """A table of 2^depth values packed 2^r = min(2^depth, N) to a sample, int32 [2^(depth-r)][k+1][N]: entry i carries encode(values[i])
    on coefficient i & (2^r - 1) of sample i >> r; coefficients past 2^r are zero.  Trivial or encrypted samples as table_to_tlwe."""
    depth, r = _packing(len(values), N)
    mu = np.zeros((1 << (depth - r), N), np.int32)
    mu[:, :1 << r] = wrap32(np.array([int(encode(v)) for v in values], np.int64)).reshape(-1, 1 << r)
    if secret_key is None:
        return tlwe_trivial(mu, k)
    if rng is None:
        raise ValueError("an encrypted table needs rng as well as secret_key")
    return tlwe_encrypt(rng, secret_key, mu)


def packed_lookup_net(depth, N):
    """The network that reads a pack_table_to_tlwe table of 2^depth entries at an address of `depth` variables (variable b = address bit
    b, bit 0 the lowest): with r = min(depth, log2 N), tree levels on the address bits r ... depth-1 fold the E = 2^(depth-r) samples to
    the one that holds the entry, then for b = 0 ... r-1 the node (0, 0, b, 0, 2N - 2^b) multiplies by X^(-2^b) where bit b is set: the
    entry arrives at coefficient 0.  E - 1 + r external products; depth 1 ... 24 while E <= 4096."""
    logN = int(N).bit_length() - 1
    if N < 2 or N != 1 << logN:
        raise ValueError(f"N = {N} (a power of two, at least 2)")
    if not 1 <= depth <= 24 or depth - min(depth, logN) > 12:
        raise ValueError(f"depth = {depth} (1 ... 24, and at most 4096 table samples: depth <= {logN + 12} at N = {N})")
    r = min(depth, logN)
    widths = [1 << (depth - r - 1 - t) for t in range(depth - r)] + [1] * r
    nodes = [(2 * i, 2 * i + 1, r + t, 0, 0) for t in range(depth - r) for i in range(widths[t])]
    nodes += [(0, 0, b, 0, 2 * N - (1 << b)) for b in range(r)]
    return RotNet(widths, nodes, N, entries=1 << (depth - r), variables=depth)


def _word_packing(count, word_bits, N):
    """depth, log2 w and r = min(depth, log2 N - log2 w) of a table of `count` = 2^depth entries of w = word_bits bits each."""
    w, logN = int(word_bits), int(N).bit_length() - 1
    if N < 2 or N != 1 << logN:
        raise ValueError(f"N = {N} (a power of two, at least 2)")
    if w < 1 or w & (w - 1) or w > N:
        raise ValueError(f"word_bits = {word_bits} (a power of two, at most N = {N})")
    depth = int(count).bit_length() - 1
    if count < 2 or count != 1 << depth:
        raise ValueError(f"a packed table has 2^depth entries (depth >= 1), got {count}")
    return depth, w, min(depth, logN - (w.bit_length() - 1))


def pack_words_to_tlwe(values, word_bits, N, k=1, encode=encode_gate_bit):
    """A table of 2^depth words of w = word_bits bits packed 2^r = min(2^depth, N / w) words to a trivial sample, int32
    [2^(depth-r)][k+1][N]: bit t of entry i is encode(values[i] >> t & 1) on coefficient w (i mod 2^r) + t of sample i >> r;
    coefficients past w 2^r are zero.  packed_words_net reads it; with w = 1 it is pack_table_to_tlwe of the entries' lowest bits."""
    depth, w, r = _word_packing(len(values), word_bits, N)
    bits = np.array([[int(encode((int(v) >> t) & 1)) for t in range(w)] for v in values], np.int64)
    mu = np.zeros((1 << (depth - r), N), np.int32)
    mu[:, :w << r] = wrap32(bits).reshape(-1, w << r)
    return tlwe_trivial(mu, k)


def packed_words_net(depth, word_bits, N):
    """The network that reads a pack_words_to_tlwe table of 2^depth words of w = word_bits bits at an address of `depth` variables: with
    r = min(depth, log2 N - log2 w), tree levels on the address bits r ... depth-1, then for b = 0 ... r-1 the node
    (0, 0, b, 0, 2N - w 2^b): the word arrives on coefficients 0 ... w-1.  For w > 1 one last level of w rotated copies of node 0 by
    X^(-t) puts bit t on coefficient 0 of output t: F = w outputs for one address walk, and the copies add no product and no noise.
    With w = 1 it is packed_lookup_net(depth, N), record for record."""
    depth = int(depth)
    _, w, r = _word_packing(1 << max(depth, 1), word_bits, N)
    if not 1 <= depth <= 24 or depth - r > 12:
        raise ValueError(f"depth = {depth} (1 ... 24, and at most 4096 table samples: depth <= {r + 12} at N = {N}, word_bits = {w})")
    widths = [1 << (depth - r - 1 - t) for t in range(depth - r)] + [1] * r
    nodes = [(2 * i, 2 * i + 1, r + t, 0, 0) for t in range(depth - r) for i in range(widths[t])]
    nodes += [(0, 0, b, 0, 2 * N - (w << b)) for b in range(r)]
    if w > 1:
        widths.append(w)
        nodes += [(0, 0, 0, (2 * N - t) % (2 * N), (2 * N - t) % (2 * N)) for t in range(w)]
    return RotNet(widths, nodes, N, entries=1 << (depth - r), variables=depth)


def wfa_net(delta0, delta1, weight0, weight1, start, steps, N, letter_var=None):
    """dfa_net with X^weight on every transition: state q moves to delta0[q] and multiplies by X^weight0[q] on letter 0, to delta1[q]
    and X^weight1[q] on letter 1 (weights taken mod 2N).  The one output is X^(sum of the weights along the path) table[end state].  A
    state whose two transitions and weights agree becomes a rotated copy.  One state looping on itself with weights 0 and 2N - 1
    rotates by minus the popcount of the letters: f(popcount) for the table polynomial sum_c f(c) X^c."""
    base = dfa_net(delta0, delta1, start, steps, letter_var)
    w0, w1 = [int(w) % (2 * N) for w in weight0], [int(w) % (2 * N) for w in weight1]
    Q = len(w0)
    if Q != base.entries or len(w1) != Q:
        raise ValueError("weight0 and weight1 must give a weight for every state")
    reach = [[int(start)]]                                           # as dfa_net: the states after j letters, sorted
    for j in range(steps - 1):
        reach.append(sorted({d[q] for q in reach[-1] for d in (delta0, delta1)}))
    rot = [(w0[q], w1[q]) for v in range(steps) for q in reach[steps - 1 - v]]
    nodes = np.concatenate([base.nodes, np.array(rot, np.int32)], axis=1)
    return RotNet(base.widths, nodes, N, entries=Q, variables=base.variables)


def rot_net_lookup(ck, data, net, bits_tgsw, out_form=2, device=0, table_index=None):
    """cmux_net_lookup for a RotNet: the network `net` on B rows of encrypted variables.  data: int32 [E][k+1][N] or [T][E][k+1][N]
    with table_index [B]; bits_tgsw: int32 [B][V][l][k+1][k+1][N].  out_form as cmux_net_lookup (extraction at coefficient 0)."""
    a = np.asarray(bits_tgsw, np.int32)
    if a.ndim != 6:
        raise ValueError(f"bits_tgsw must be [B][V][l][k+1][k+1][N], got {a.shape}")
    B, V = a.shape[:2]
    eng = ck.engine(device)
    eng.tgsw_load(a.reshape((B * V,) + a.shape[2:]))
    sel = np.arange(B * V, dtype=np.int32).reshape(B, V)
    out = eng.rot_net(data, net, sel, table_index=table_index, out_form=out_form)
    return LweSampleArray(out.reshape(-1, out.shape[-1])) if out_form == 2 else out


def packed_lookup(ck, table, address_tgsw, out_form=2, device=0, encode=encode_gate_bit):
    """table[address] for B encrypted addresses through a packed table: cmux_lookup at 2^(d - log2 N) - 1 + log2 N external products per
    address.  table: 2^d plain values (packed here by pack_table_to_tlwe as trivial samples) or the packed samples themselves, int32
    [2^(d-r)][k+1][N]; address_tgsw: int32 [B][d][l][k+1][k+1][N] as cmux_lookup's.  out_form 2 (default): an LweSampleArray of B
    samples under the gate key; 1: extracted [B][k N + 1]; 0: the TLWE samples [B][k+1][N], the entry on coefficient 0."""
    a = np.asarray(address_tgsw, np.int32)
    if a.ndim != 6:
        raise ValueError(f"address_tgsw must be [B][depth][l][k+1][k+1][N], got {a.shape}")
    depth, N, k = a.shape[1], a.shape[-1], a.shape[3] - 1
    t = np.asarray(table)
    data = pack_table_to_tlwe(list(t), N, k, encode) if t.ndim == 1 else t
    net = packed_lookup_net(depth, N)
    if data.shape[0] != net.entries:
        raise ValueError(f"a packed table of 2^{depth} entries has {net.entries} samples, got {data.shape[0]}")
    out = rot_net_lookup(ck, data, net, a, out_form=out_form, device=device)
    return out if out_form == 2 else out[:, 0]


# ---- the blind rotation of the caller's accumulators: private tables, two-stage lookups, gate outputs as table entries ------------
def bootstrap_key_selectors(ck):
    """The bootstrapping key of the CloudKey ck as a selector set for Engine.tgsw_load: int32 [n][l][k+1][k+1][N], selector i the TGSW
    encryption of bit i of the LWE key (bootstrap.jl:6-15) — the rotation key of Engine.blind_rotate with sel None."""
    p = ck.params
    return np.ascontiguousarray(ck.bootstrap_key, np.int32).reshape(p.lwe_size, p.bs_decomp_length, p.tlwe_mask_size + 1, p.tlwe_mask_size + 1,
                                                                    p.tlwe_polynomial_degree)


def private_lut_encrypt(rng, secret_key, f, p, q=None):
    """A private lookup table: tlwe_encrypt of lut.make_test_vector(f, p, N, q), int32 [1][k+1][N] under secret_key.tlwe_key.  Rotated
    by lut_encrypt(m, p) (blind_rotate_lookup) it returns f(m) in Z_q, and the server never sees f."""
    return tlwe_encrypt(rng, secret_key, make_test_vector(f, p, _tlwe_key(secret_key).N, q))


def _lwe_rows(lwe):
    return lwe.data if isinstance(lwe, LweSampleArray) else np.asarray(lwe, np.int32)


def _tuned_engine(ck, device):
    """ck's engine where Engine.bootstrap_acc serves its shape and key layout (option "bootstrap_acc"); ValueError elsewhere."""
    eng = ck.engine(device)
    if not eng.get_option("bootstrap_acc"):
        p = ck.params
        raise ValueError(f"tuned=True: Engine.bootstrap_acc serves N = 1024, k = 1 in the gates' key layout; this context has "
                         f"N = {p.tlwe_polynomial_degree}, k = {p.tlwe_mask_size} (option bootstrap_acc is 0): use tuned=False")
    return eng


def blind_rotate_lookup(ck, acc, lwe, extra_tgsw=None, acc_index=None, n_out=1, out_form=2, device=0, tuned=False):
    """acc[acc_index[g]] rotated by row g of `lwe` under ck's bootstrapping key (Engine.blind_rotate with in_form 0).  Loads the key's n
    entries as selectors 0 ... n-1 and, behind them, the `extra_tgsw` samples int32 [E][l][k+1][k+1][N] (address bits for a later
    cmux_tree on the same engine: selectors n ... n+E-1), once; then rotates.  acc: int32 [T][k+1][N] (or [k+1][N]); lwe: an
    LweSampleArray or int32 [B][n+1].  out_form 2 (default): an LweSampleArray of B n_out samples under the gate key (row g's output j
    at g n_out + j); 1: extracted int32 [B][n_out][k N + 1]; 0: the TLWE samples int32 [B][k+1][N].
    tuned=True: the same words from Engine.bootstrap_acc, on the gates' own kernel and key; only `extra_tgsw` is loaded as the
    selector set (selectors 0 ... E-1).  ValueError where get_option("bootstrap_acc") is 0."""
    if tuned:
        eng = _tuned_engine(ck, device)
        if extra_tgsw is not None:
            eng.tgsw_load(np.asarray(extra_tgsw, np.int32))
        out = eng.bootstrap_acc(acc, _lwe_rows(lwe), acc_index=acc_index, n_out=n_out, out_form=out_form)
        return LweSampleArray(out.reshape(-1, out.shape[-1])) if out_form == 2 else out
    eng = ck.engine(device)
    sels = bootstrap_key_selectors(ck)
    if extra_tgsw is not None:
        extra = np.asarray(extra_tgsw, np.int32)
        if extra.ndim != 5 or extra.shape[1:] != sels.shape[1:]:
            raise ValueError(f"extra_tgsw must be [E]{list(sels.shape[1:])}, got {extra.shape}")
        sels = np.concatenate([sels, extra])
    eng.tgsw_load(sels)
    sel = None if extra_tgsw is None else np.arange(ck.params.lwe_size, dtype=np.int32)
    out = eng.blind_rotate(acc, _lwe_rows(lwe), sel=sel, acc_index=acc_index, in_form=0, n_out=n_out, out_form=out_form)
    return LweSampleArray(out.reshape(-1, out.shape[-1])) if out_form == 2 else out


def two_stage_lookup(ck, tables, high_bits_tgsw, low_lwe, p, out_form=2, device=0, tuned=False):
    """A table of p 2^d entries addressed by d TGSW-encrypted high bits and one LWE digit of Z_p that gates or lookups computed.
    tables: int32 [2^d][k+1][N], sample h the test polynomial (trivial: tlwe_trivial(make_test_vector(...)); or private_lut_encrypt) of
    the p entries whose high address is h; high_bits_tgsw: int32 [B][d][l][k+1][k+1][N], bit v of row g (bit 0 the lowest); low_lwe: an
    LweSampleArray or int32 [B][n+1] of messages in Z_p (lut_encode).  A CMUX tree with out_form 0 picks row g's sample, the rotation
    by its low digit reads the entry: 2^d - 1 external products plus one rotation per row.  out_form as blind_rotate_lookup (n_out 1).
    tuned=True: the rotation by Engine.bootstrap_acc, the selector set holding the address bits alone (blind_rotate_lookup)."""
    a = np.asarray(high_bits_tgsw, np.int32)
    if a.ndim != 6:
        raise ValueError(f"high_bits_tgsw must be [B][depth][l][k+1][k+1][N], got {a.shape}")
    B, depth = a.shape[:2]
    rows = _lwe_rows(low_lwe)
    if rows.shape[0] != B:
        raise ValueError(f"low_lwe has {rows.shape[0]} rows, high_bits_tgsw {B}")
    if int(p) < 2 or int(p) & (int(p) - 1) or int(p) > a.shape[-1] // 2:
        raise ValueError(f"p = {p} (a power of two, 2 ... N/2)")
    n = ck.params.lwe_size
    if tuned:
        eng = _tuned_engine(ck, device)
        eng.tgsw_load(a.reshape((B * depth,) + a.shape[2:]))
        picked = eng.cmux_tree(tables, np.arange(B * depth, dtype=np.int32).reshape(B, depth), out_form=0)
        out = eng.bootstrap_acc(picked, rows, acc_index=np.arange(B, dtype=np.int32), out_form=out_form)
        return LweSampleArray(out.reshape(-1, out.shape[-1])) if out_form == 2 else out
    eng = ck.engine(device)
    eng.tgsw_load(np.concatenate([bootstrap_key_selectors(ck), a.reshape((B * depth,) + a.shape[2:])]))
    picked = eng.cmux_tree(tables, n + np.arange(B * depth, dtype=np.int32).reshape(B, depth), out_form=0)
    out = eng.blind_rotate(picked, rows, sel=np.arange(n, dtype=np.int32), acc_index=np.arange(B, dtype=np.int32), in_form=0, out_form=out_form)
    return LweSampleArray(out.reshape(-1, out.shape[-1])) if out_form == 2 else out


def pbs_to_tlwe(ck, lwe, f, p, q=None, device=0, tuned=False):
    """f(m) of every sample of m in Z_p as a TLWE sample int32 [B][k+1][N]: the rotation of the trivial accumulator (0, test vector)
    with out_form 0.  The test polynomial is constant over each window, so coefficient 0 carries lut_encode(f(m), q) — where
    cmux_lookup / cmux_net_lookup read their `data` and extract: a gate or lookup output becomes a table entry with no packing key and
    no keyswitch noise.  f: a callable Z_p -> Z_q or an int32 test polynomial [N].  tuned: as blind_rotate_lookup."""
    N, k = ck.params.tlwe_polynomial_degree, ck.params.tlwe_mask_size
    tv = make_test_vector(f, p, N, q) if callable(f) else np.asarray(f, np.int32)
    return blind_rotate_lookup(ck, tlwe_trivial(tv, k), lwe, out_form=0, device=device, tuned=tuned)


# ---- under a multi-key cloud key -------------------------------------------------------------------------------------------------
def mk_tlwe_trivial(polys, parties):
    """mk_tlwe_noiseless_trivial (mk_internals.jl:69-76) of each message polynomial: int32 [..., N] -> int32 [count][P+1][N], zero masks."""
    return tlwe_trivial(polys, parties)


def _mk_tlwe_keys(tlwe_keys):
    if any(k is None for k in tlwe_keys):
        raise ValueError("a party's TLWE key is missing: CloudKeyPart(rng, secret_key, shared_key, keep_tlwe_key=True) keeps it as .tlwe_key")
    return np.stack([k.key[0] for k in tlwe_keys])                       # [P][N] (mask_size = 1, mk_internals.jl:129)


def mk_tlwe_encrypt(rng, tlwe_keys, alpha, polys):
    """An MKTLweSample (mk_internals.jl:46-57) of each Torus32 message polynomial under the P parties' TLWE keys: uniform masks a_p,
    b = sum_p a_p (*) s_p + e + mu with Gaussian e of standard deviation alpha; int32 [..., N] -> int32 [count][P+1][N]."""
    s = _mk_tlwe_keys(tlwe_keys)
    P, N = s.shape
    mu = np.atleast_2d(np.asarray(polys, np.int32))
    if mu.shape[1] != N:
        raise ValueError(f"message polynomials must have {N} coefficients, got {mu.shape[1]}")
    a = rand_uniform_torus32(rng, mu.shape[0], P, N)
    b = mu.astype(np.int64) + dtot32(rng.standard_normal(size=mu.shape) * alpha).astype(np.int64)
    for p in range(P):
        b = b + negacyclic_mul_binary(s[p], a[:, p, :]).astype(np.int64)
    return np.concatenate([a, wrap32(b)[:, None, :]], axis=1).astype(np.int32)


def mk_tlwe_phase(tlwe_keys, samples):
    """b - sum_p a_p (*) s_p (negacyclic) of MK TLWE samples int32 [count][P+1][N]: the noisy message polynomials [count][N]."""
    s = _mk_tlwe_keys(tlwe_keys)
    P = s.shape[0]
    x = np.asarray(samples, np.int32)
    if x.ndim == 2:
        x = x[None]
    ph = x[:, P, :].astype(np.int64)
    for p in range(P):
        ph = ph - negacyclic_mul_binary(s[p], x[:, p, :]).astype(np.int64)
    return wrap32(ph)


def mk_tgsw_uni_encrypt_bits(rng, tlwe_key, shared_key, public_b, bits):
    """mk_tgsw_encrypt (RGSW.UniEnc, mk_internals.jl:185-227) of each bit at bs_noise_stddev under one party's TLWE key and public key
    public_b [l][N]: the six arrays (c0, c1, d0, d1, f0, f1), int32 [S][l][N] each — what CloudKeyPart makes of its LWE key's bits."""
    m = np.asarray(bits).astype(bool).reshape(-1).astype(np.int64)
    return mk_keys._uni_encrypt(rng, shared_key.params, tlwe_key.key[0], shared_key.a, public_b, m)


def mk_tgsw_expand(params, public_bs, party, c0, c1, d0, d1, f0, f1):
    """mk_tgsw_expand (RGSW.Expand, mk_internals.jl:304-345) of one party's uni-encryptions [S][l][N] against all public keys
    public_bs [P][l][N]: int32 [S][2lP + 2l][N], each sample x[l][P] | y[l][P] | c0[l] | c1[l] as an entry of the multi-key
    bootstrapping key (MKCloudKey expands its parts through the same function)."""
    return mk_keys._expand(params, list(public_bs), int(party), *(np.asarray(v, np.int32) for v in (c0, c1, d0, d1, f0, f1)))


def mk_cmux_lookup(ck, tables, uni_bits, party_of, out_form=2, expand="device", device=0, table_index=None):
    """table[address] for B jointly encrypted addresses under the MKCloudKey ck.  tables: int32 [2^d][P+1][N] or [T][2^d][P+1][N] with
    table_index [B]; uni_bits: the six arrays of mk_tgsw_uni_encrypt_bits, each [B][d][l][N], bit v of address g uni-encrypted by party
    party_of[g][v] (party_of: [B][d], or [d] for every row).  expand "device": RGSW.Expand on the GPU (tfhe_mk_tgsw_expand_load),
    "host": numpy (mk_tgsw_expand) then mk_tgsw_load.  out_form 2 (default): multi-key LWE samples int32 [B][P*n+1] for mk_decrypt /
    mk_gate_*; 1: extracted [B][P*N+1]; 0: MK TLWE samples [B][P+1][N]."""
    eng, sel = _mk_load_selectors(ck, uni_bits, party_of, expand, device, "depth")
    return eng.mk_cmux_tree(tables, sel, table_index=table_index, out_form=out_form)


def _mk_load_selectors(ck, uni_bits, party_of, expand, device, what):
    """Expand B rows of C uni-encrypted bits (six arrays [B][C][l][N], bit c of row g by party party_of[g][c]) into the selector set of
    ck's engine on `device`, on the GPU or in numpy.  Returns the engine and sel [B][C], row g's selectors in order."""
    assert expand in ("device", "host")
    arrs = [np.asarray(a, np.int32) for a in uni_bits]
    if len(arrs) != 6 or arrs[0].ndim != 4 or any(a.shape != arrs[0].shape for a in arrs):
        raise ValueError(f"uni_bits must be six arrays [B][{what}][l][N]")
    B, C = arrs[0].shape[:2]
    who = np.broadcast_to(np.asarray(party_of, np.int32), (B, C)).reshape(-1)
    flat = [a.reshape((B * C,) + a.shape[2:]) for a in arrs]
    pub = np.stack([part.public_b for part in ck._parts])
    eng = ck.engine(device)
    if expand == "device":
        eng.mk_tgsw_expand_load(pub, who, *flat)
    else:
        tg = np.zeros((B * C, 2 * arrs[0].shape[2] * (ck.parties + 1), arrs[0].shape[3]), np.int32)
        for i in range(ck.parties):
            mine = np.nonzero(who == i)[0]
            if mine.size:
                tg[mine] = mk_tgsw_expand(ck.params, pub, i, *[a[mine] for a in flat])
        eng.mk_tgsw_load(tg, who)
    return eng, np.arange(B * C, dtype=np.int32).reshape(B, C)


def mk_cmux_net_lookup(ck, data, net, uni_bits, party_of, out_form=2, expand="device", device=0, table_index=None):
    """The network `net` on B rows of jointly encrypted variables under the MKCloudKey ck (Engine.mk_cmux_net, tfhe_mk_cmux_net_batch).
    data: int32 [E][P+1][N] or [T][E][P+1][N] with table_index [B]; the table of an automaton under P parties is
    table_to_tlwe(values, N, k=P): trivial samples with P zero masks.  uni_bits: the six arrays of mk_tgsw_uni_encrypt_bits, each
    [B][V][l][N], variable v of row g uni-encrypted by party party_of[g][v] (party_of: [B][V], or [V] for every row); expand as
    mk_cmux_lookup.  With less_than_net(d), party 0 owning x (variables 0 ... d-1) and party 1 owning y (d ... 2d-1), the one output
    is x < y and neither party shows its integer.  out_form 2 (default): multi-key LWE samples int32 [B F][P*n+1] for mk_decrypt /
    mk_gate_* (row g's output i at g F + i; F = 1 for an automaton); 1: extracted [B][F][P*N+1]; 0: MK TLWE samples [B][F][P+1][N]."""
    eng, sel = _mk_load_selectors(ck, uni_bits, party_of, expand, device, "V")
    out = eng.mk_cmux_net(data, net, sel, table_index=table_index, out_form=out_form)
    return out.reshape(-1, out.shape[-1]) if out_form == 2 else out


def mk_rot_net_lookup(ck, data, net, uni_bits, party_of, out_form=2, expand="device", device=0, table_index=None):
    """mk_cmux_net_lookup for a RotNet (Engine.mk_rot_net, tfhe_mk_rot_net_batch): the network `net` on B rows of jointly encrypted
    variables.  data: int32 [E][P+1][N] or [T][E][P+1][N] with table_index [B]; uni_bits, party_of, expand and out_form as
    mk_cmux_net_lookup (extraction at coefficient 0)."""
    eng, sel = _mk_load_selectors(ck, uni_bits, party_of, expand, device, "V")
    out = eng.mk_rot_net(data, net, sel, table_index=table_index, out_form=out_form)
    return out.reshape(-1, out.shape[-1]) if out_form == 2 else out


def mk_packed_lookup(ck, table, uni_bits, party_of, out_form=2, expand="device", device=0, encode=encode_gate_bit):
    """table[address] for B jointly encrypted addresses through a packed table: mk_cmux_lookup at 2^(d - log2 N) - 1 + log2 N external
    products per address.  table: 2^d plain values (packed here by pack_table_to_tlwe(values, N, k=P) as trivial samples) or the packed
    MK TLWE samples themselves, int32 [2^(d-r)][P+1][N]; uni_bits: the six arrays of mk_tgsw_uni_encrypt_bits, each [B][d][l][N], bit v
    of address g uni-encrypted by party party_of[g][v].  out_form 2 (default): multi-key LWE samples int32 [B][P*n+1] for mk_decrypt /
    mk_gate_*; 1: extracted [B][P*N+1]; 0: the MK TLWE samples [B][P+1][N], the entry on coefficient 0."""
    shape = np.shape(uni_bits[0]) if len(uni_bits) == 6 else ()
    if len(shape) != 4:
        raise ValueError("uni_bits must be six arrays [B][depth][l][N]")
    depth, N = shape[1], shape[3]
    t = np.asarray(table)
    data = pack_table_to_tlwe(list(t), N, ck.parties, encode) if t.ndim == 1 else t
    net = packed_lookup_net(depth, N)
    if data.shape[0] != net.entries:
        raise ValueError(f"a packed table of 2^{depth} entries has {net.entries} samples, got {data.shape[0]}")
    out = mk_rot_net_lookup(ck, data, net, uni_bits, party_of, out_form=out_form, expand=expand, device=device)
    return out if out_form == 2 else out[:, 0]


# ---- the multi-key blind rotation of the caller's accumulators: one party's private table on jointly encrypted data ----------------
def mk_bootstrap_key_selectors(ck):
    """The bootstrapping key of the MKCloudKey ck as a selector set for Engine.mk_tgsw_load: (tgsw int32 [P n][2lP + 2l][N], party_of
    int32 [P n]), party-major — selector i n + j the expanded RGSW encryption of bit j of party i's LWE key (mk_internals.jl:419-439),
    the rotation key of Engine.mk_blind_rotate with sel None: a multi-key LWE sample's words line up with it."""
    bk = np.ascontiguousarray(ck.bootstrap_key, np.int32)
    P, n = bk.shape[:2]
    return bk.reshape((P * n,) + bk.shape[2:]), np.repeat(np.arange(P, dtype=np.int32), n)


def mk_private_lut_encrypt(rng, tlwe_keys, alpha, f, p, q=None):
    """A private lookup table under P parties' TLWE keys: mk_tlwe_encrypt of lut.make_test_vector(f, p, N, q), int32 [1][P+1][N].
    Rotated by mk_lut_encrypt(m, p) (mk_blind_rotate_lookup) it returns f(m) in Z_q, and the server never sees f."""
    return mk_tlwe_encrypt(rng, tlwe_keys, alpha, make_test_vector(f, p, tlwe_keys[0].N, q))


def _mk_load_key_selectors(ck, extra_uni_bits, extra_party_of, expand, device):
    """ck's P n bootstrapping-key entries as selectors 0 ... P n - 1 of its engine on `device` and, behind them, the E samples of
    extra_uni_bits (six arrays [E][l][N], sample e uni-encrypted by party extra_party_of[e]).  expand "device": RGSW.Expand of the
    parts' uni-encryptions and the extra ones on the GPU; "host": the key's host expansion and mk_tgsw_expand.  Returns the engine."""
    assert expand in ("device", "host")
    P, n = ck.parties, ck.params.lwe_size
    extra, who_extra = None, np.zeros(0, np.int32)
    if extra_uni_bits is not None:
        extra = [np.asarray(a, np.int32) for a in extra_uni_bits]
        if len(extra) != 6 or extra[0].ndim != 3 or any(a.shape != extra[0].shape for a in extra):
            raise ValueError("extra_uni_bits must be six arrays [E][l][N]")
        who_extra = np.asarray(extra_party_of, np.int32).reshape(-1)
        if who_extra.size != extra[0].shape[0]:
            raise ValueError(f"extra_party_of must have one entry per extra sample ({extra[0].shape[0]}), got {who_extra.size}")
    who = np.concatenate([np.repeat(np.arange(P, dtype=np.int32), n), who_extra])
    pub = np.stack([part.public_b for part in ck._parts])
    eng = ck.engine(device)
    if expand == "device":
        flat = [a.reshape((P * n,) + a.shape[2:]) for a in ck._part_arrays()[1:]]
        if extra is not None:
            flat = [np.concatenate([a, b]) for a, b in zip(flat, extra)]
        eng.mk_tgsw_expand_load(pub, who, *flat)
    else:
        tg = mk_bootstrap_key_selectors(ck)[0]
        if extra is not None:
            more = np.zeros((who_extra.size,) + tg.shape[1:], np.int32)
            for i in range(P):
                mine = np.nonzero(who_extra == i)[0]
                if mine.size:
                    more[mine] = mk_tgsw_expand(ck.params, pub, i, *[a[mine] for a in extra])
            tg = np.concatenate([tg, more])
        eng.mk_tgsw_load(tg, who)
    eng._mk_key_extra = int(who_extra.size)      # (mk_two_stage_lookup_device: the key is resident with this many selectors behind it)
    return eng


def _mk_tuned_engine(ck, device):
    """ck's engine where Engine.mk_bootstrap_acc serves its shape and key layout (option "mk_bootstrap_acc"); ValueError elsewhere."""
    eng = ck.engine(device)
    if not eng.get_option("mk_bootstrap_acc"):
        p = ck.params
        raise ValueError(f"tuned=True: Engine.mk_bootstrap_acc serves 2 parties, N = 1024, l = 4 in the gates' key layout; this context has "
                         f"{ck.parties} parties, N = {p.tlwe_polynomial_degree}, l = {p.bs_decomp_length} (option mk_bootstrap_acc is 0): use tuned=False")
    return eng


def _mk_load_extra_selectors(ck, extra_uni_bits, extra_party_of, expand, device):
    """The tuned rotation's selector set: the E samples of extra_uni_bits alone, as selectors 0 ... E - 1 of ck's engine on `device` (the
    bootstrapping key is read in the gates' layout and is not loaded as selectors); nothing is loaded without extra bits.  Returns the
    engine."""
    assert expand in ("device", "host")
    eng = _mk_tuned_engine(ck, device)
    if extra_uni_bits is None:
        return eng
    extra = [np.asarray(a, np.int32) for a in extra_uni_bits]
    if len(extra) != 6 or extra[0].ndim != 3 or any(a.shape != extra[0].shape for a in extra):
        raise ValueError("extra_uni_bits must be six arrays [E][l][N]")
    who = np.ascontiguousarray(np.asarray(extra_party_of, np.int32).reshape(-1))
    if who.size != extra[0].shape[0]:
        raise ValueError(f"extra_party_of must have one entry per extra sample ({extra[0].shape[0]}), got {who.size}")
    pub = np.stack([part.public_b for part in ck._parts])
    if expand == "device":
        eng.mk_tgsw_expand_load(pub, who, *extra)
    else:
        l, N = extra[0].shape[1:]
        tg = np.zeros((who.size, 2 * l * ck.parties + 2 * l, N), np.int32)
        for i in range(ck.parties):
            mine = np.nonzero(who == i)[0]
            if mine.size:
                tg[mine] = mk_tgsw_expand(ck.params, pub, i, *[a[mine] for a in extra])
        eng.mk_tgsw_load(tg, who)
    eng._mk_key_extra = ("tuned", int(who.size))      # (mk_two_stage_lookup_device: this many selectors are resident, without the key)
    return eng


def mk_blind_rotate_lookup(ck, acc, lwe, extra_uni_bits=None, extra_party_of=None, acc_index=None, n_out=1, out_form=2, expand="device", device=0,
                           tuned=False):
    """acc[acc_index[g]] rotated by row g of `lwe` under the MKCloudKey ck's bootstrapping key (Engine.mk_blind_rotate with in_form 0).
    Loads the key's P n entries as selectors 0 ... P n - 1 and, behind them, the extra address bits (six arrays [E][l][N] of
    mk_tgsw_uni_encrypt_bits, sample e by party extra_party_of[e]: selectors P n ... P n + E - 1, for a later mk_cmux_tree on the same
    engine), once; then rotates.  expand "device": RGSW.Expand on the GPU (tfhe_mk_tgsw_expand_load) of the parts' uni-encryptions,
    "host": the host expansion then mk_tgsw_load.  acc: int32 [T][P+1][N] (or [P+1][N]); lwe: int32 [B][P n + 1].  out_form 2
    (default): multi-key LWE samples int32 [B n_out][P*n+1] for mk_decrypt / mk_gate_* (row g's output j at g n_out + j); 1: extracted
    int32 [B][n_out][P*N+1]; 0: the MK TLWE samples int32 [B][P+1][N].
    tuned=True: the same words from Engine.mk_bootstrap_acc, on the multi-key gates' own kernel and key; the key is not loaded as
    selectors, only the extra address bits are (selectors 0 ... E-1).  ValueError where get_option("mk_bootstrap_acc") is 0."""
    if tuned:
        eng = _mk_load_extra_selectors(ck, extra_uni_bits, extra_party_of, expand, device)
        out = eng.mk_bootstrap_acc(acc, np.asarray(lwe, np.int32), acc_index=acc_index, n_out=n_out, out_form=out_form)
        return out.reshape(-1, out.shape[-1]) if out_form == 2 else out
    eng = _mk_load_key_selectors(ck, extra_uni_bits, extra_party_of, expand, device)
    sel = None if extra_uni_bits is None else np.arange(ck.parties * ck.params.lwe_size, dtype=np.int32)
    out = eng.mk_blind_rotate(acc, np.asarray(lwe, np.int32), sel=sel, acc_index=acc_index, in_form=0, n_out=n_out, out_form=out_form)
    return out.reshape(-1, out.shape[-1]) if out_form == 2 else out


def mk_two_stage_lookup(ck, tables, high_uni_bits, party_of, low_lwe, p, out_form=2, expand="device", device=0, tuned=False):
    """A table of p 2^d entries addressed by d jointly encrypted high bits and one multi-key LWE digit of Z_p that gates or lookups
    computed.  tables: int32 [2^d][P+1][N], sample h the test polynomial (trivial: mk_tlwe_trivial(make_test_vector(...), P); or
    mk_private_lut_encrypt) of the p entries whose high address is h; high_uni_bits: the six arrays of mk_tgsw_uni_encrypt_bits, each
    [B][d][l][N], bit v of row g (bit 0 the lowest) uni-encrypted by party party_of[g][v] (party_of: [B][d], or [d] for every row);
    low_lwe: int32 [B][P n + 1] of messages in Z_p (mk_lut_encrypt).  An MK CMUX tree with out_form 0 picks row g's sample, the
    rotation by its low digit reads the entry: 2^d - 1 MK external products plus one MK rotation per row.  out_form as
    mk_blind_rotate_lookup (n_out 1).
    tuned=True: the rotation by Engine.mk_bootstrap_acc, the selector set holding the address bits alone (mk_blind_rotate_lookup)."""
    arrs = [np.asarray(a, np.int32) for a in high_uni_bits]
    if len(arrs) != 6 or arrs[0].ndim != 4 or any(a.shape != arrs[0].shape for a in arrs):
        raise ValueError("high_uni_bits must be six arrays [B][depth][l][N]")
    B, depth = arrs[0].shape[:2]
    rows = np.asarray(low_lwe, np.int32)
    if rows.shape[0] != B:
        raise ValueError(f"low_lwe has {rows.shape[0]} rows, high_uni_bits {B}")
    if int(p) < 2 or int(p) & (int(p) - 1) or int(p) > arrs[0].shape[-1] // 2:
        raise ValueError(f"p = {p} (a power of two, 2 ... N/2)")
    who = np.broadcast_to(np.asarray(party_of, np.int32), (B, depth)).reshape(-1)
    Pn = ck.parties * ck.params.lwe_size
    if tuned:
        eng = _mk_load_extra_selectors(ck, [a.reshape((B * depth,) + a.shape[2:]) for a in arrs], who, expand, device)
        picked = eng.mk_cmux_tree(tables, np.arange(B * depth, dtype=np.int32).reshape(B, depth), out_form=0)
        out = eng.mk_bootstrap_acc(picked, rows, acc_index=np.arange(B, dtype=np.int32), out_form=out_form)
        return out.reshape(-1, out.shape[-1]) if out_form == 2 else out
    eng = _mk_load_key_selectors(ck, [a.reshape((B * depth,) + a.shape[2:]) for a in arrs], who, expand, device)
    picked = eng.mk_cmux_tree(tables, Pn + np.arange(B * depth, dtype=np.int32).reshape(B, depth), out_form=0)
    out = eng.mk_blind_rotate(picked, rows, sel=np.arange(Pn, dtype=np.int32), acc_index=np.arange(B, dtype=np.int32), in_form=0, out_form=out_form)
    return out.reshape(-1, out.shape[-1]) if out_form == 2 else out


def mk_pbs_to_tlwe(ck, lwe, f, p, q=None, device=0, tuned=False):
    """f(m) of every multi-key sample of m in Z_p as an MK TLWE sample int32 [B][P+1][N]: the rotation of the trivial accumulator
    (0, ..., 0, test vector) with out_form 0.  The test polynomial is constant over each window, so coefficient 0 carries
    lut_encode(f(m), q) — where mk_cmux_lookup / mk_cmux_net_lookup read their `data` and extract: a multi-key gate or lookup output
    becomes a table entry with no packing key and no keyswitch noise.  f: a callable Z_p -> Z_q or an int32 test polynomial [N].
    tuned: as mk_blind_rotate_lookup."""
    N = ck.params.tlwe_polynomial_degree
    tv = make_test_vector(f, p, N, q) if callable(f) else np.asarray(f, np.int32)
    return mk_blind_rotate_lookup(ck, mk_tlwe_trivial(tv, ck.parties), lwe, out_form=0, device=device, tuned=tuned)


def mk_two_stage_lookup_device(ck, table_slot, high_uni_bits, party_of, low_wires, out_wires, work_slot, device=0, tuned=False):
    """mk_two_stage_lookup between the device-resident tables of ck's engine: the 2^d test polynomials are in MK TLWE slots
    [table_slot, table_slot + 2^d) (Engine.mk_tlwe_upload), row g's low digit is multi-key wire low_wires[g] (what mk_lut_level or
    mk_gates_level left there) and its answer goes, keyswitched, to wire out_wires[g]; slots [work_slot, work_slot + B) receive the
    picked samples.  The key's P n selectors are loaded once per engine, with the first request's address bits behind them
    (tfhe_mk_tgsw_expand_load); every later request of the same shape swaps only its B d address bits in (Engine.mk_tgsw_expand_update)
    instead of re-expanding the key.  Then Engine.mk_rot_net_level (the tree, into slots) and Engine.mk_blind_rotate_level (into wires):
    nothing but the uni-encryptions and the index maps crosses PCIe.  The words in out_wires equal mk_two_stage_lookup's on the same
    samples.  Returns the engine.
    tuned=True: the rotation by Engine.mk_bootstrap_acc_level on the multi-key gates' own kernel and key: the key is never loaded as
    selectors, the set holds the B d address bits alone (selectors 0 ... B d - 1), swapped in place by later requests of the same shape.
    The same words; ValueError where get_option("mk_bootstrap_acc") is 0."""
    arrs = [np.asarray(a, np.int32) for a in high_uni_bits]
    if len(arrs) != 6 or arrs[0].ndim != 4 or any(a.shape != arrs[0].shape for a in arrs):
        raise ValueError("high_uni_bits must be six arrays [B][depth][l][N]")
    B, depth = arrs[0].shape[:2]
    low = np.asarray(low_wires, np.int32).reshape(-1)
    if low.size != B:
        raise ValueError(f"low_wires has {low.size} entries, high_uni_bits {B} rows")
    who = np.ascontiguousarray(np.broadcast_to(np.asarray(party_of, np.int32), (B, depth)).reshape(-1))
    flat = [a.reshape((B * depth,) + a.shape[2:]) for a in arrs]
    Pn = ck.parties * ck.params.lwe_size
    if tuned:
        eng = _mk_tuned_engine(ck, device)
        if getattr(eng, "_mk_key_extra", None) == ("tuned", B * depth):
            eng.mk_tgsw_expand_update(0, np.stack([part.public_b for part in ck._parts]), who, *flat)
        else:
            _mk_load_extra_selectors(ck, flat, who, "device", device)
        eng.mk_rot_net_level(tree_net(depth), np.arange(B * depth, dtype=np.int32).reshape(B, depth), table_first=np.full(B, int(table_slot), np.int32),
                             out_form=0, out_first=int(work_slot))
        eng.mk_bootstrap_acc_level(int(work_slot) + np.arange(B, dtype=np.int32), np.arange(B + 1, dtype=np.int32), low, np.ones(B, np.int32),
                                   out_form=2, out_wires=out_wires)
        return eng
    eng = ck.engine(device)
    if getattr(eng, "_mk_key_extra", None) == B * depth:
        eng.mk_tgsw_expand_update(Pn, np.stack([part.public_b for part in ck._parts]), who, *flat)
    else:
        _mk_load_key_selectors(ck, flat, who, "device", device)
    eng.mk_rot_net_level(tree_net(depth), Pn + np.arange(B * depth, dtype=np.int32).reshape(B, depth), table_first=np.full(B, int(table_slot), np.int32),
                         out_form=0, out_first=int(work_slot))
    eng.mk_blind_rotate_level(int(work_slot) + np.arange(B, dtype=np.int32), np.arange(B + 1, dtype=np.int32), low, np.ones(B, np.int32),
                              sel=np.arange(Pn, dtype=np.int32), out_form=2, out_wires=out_wires)
    return eng
