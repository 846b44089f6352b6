"""CMUX networks of the leveled mode (tfhe_cmux_net_batch; tfhe_jl_amd.leveled.CmuxNet, tree_net, dfa_net, less_than_net) against an
integer schoolbook network.

The reference of every word comparison is `net_ref` below: tests/test_leveled.py's `Tree.cmux` (exact int64, np.convolve, no transform,
no rounding) per node, a copy node copying — never the engine.  Operands come from test_leveled's `_setup`: arbitrary Int32 words with
the extreme rows where the set is exact for any words (exact_domain 2), real encryptions elsewhere.

Noise (why "all 8 comparisons correct" at full size is a condition, not a measurement): the comparator's accepting path crosses at most
one non-copy node per level, 32 levels for 16-bit operands, each adding one external product's noise (3e-4 of the torus at
tfhe_parameters_80, tests/test_leveled.py) to a window of 1/8; the schoolbook network alone gave 8 of 8 there with the worst phase error
4.1e-3 of the torus, 30 times inside the window.
"""
import ctypes as C

import numpy as np
import pytest

from test_leveled import LWE_N as LWE, Tree, _params, _setup, _words

INVALID, NO_KEY, STATE, NOMEM = 1, 3, 5, 6


def net_ref(ref, net, table, sels):
    """The schoolbook network: `ref` a Tree over the selector set, `table` [E][k+1][N], sels[var] the selector behind each variable of
    the row.  Returns the outputs of the last level, int64 [F][k+1][N]."""
    cur = [np.asarray(t, np.int64) for t in table]
    for v in range(net.levels):
        cur = [cur[s0].copy() if s0 == s1 else ref.cmux(sels[var], cur[s0], cur[s1]) for s0, s1, var in net.level(v).tolist()]
    return np.stack(cur)


def ref_rows(ref, net, data, rows, sel):
    want = np.stack([net_ref(ref, net, data[rows[g]], sel[g]) for g in range(len(sel))])                 # [B][F][k+1][N]
    ext = np.stack([[ref.extract(w) for w in row] for row in want]).astype(np.int32)                      # [B][F][kN+1]
    return want.astype(np.int32), ext


def random_net(rng, E, widths, V):
    """Random sources and per-node variables; planted: a copy node at level 0 and one at the last level (the copy path with and without
    the extraction), a node with src0 > src1, and no other copies."""
    nodes = []
    for v, w in enumerate(widths):
        below = E if v == 0 else widths[v - 1]
        for i in range(w):
            s0 = int(rng.integers(0, below))
            s1 = int((s0 + 1 + rng.integers(0, below - 1)) % below)
            nodes.append([s0, s1, int(rng.integers(0, V))])
    nodes[0][:2] = [2, 2]
    nodes[1][:2] = [4, 1]
    nodes[-1][1] = nodes[-1][0]
    nodes[2][2], nodes[3][2] = 0, V - 1                                # level 0 mixes variables
    return nodes


# ---- 1. CPU: the builders, the validation, the reference itself -------------------------------------------------------------------
def test_less_than_net_clear_equals_comparison_for_all_pairs(tfhe):
    from tfhe_jl_amd import leveled
    net, table = leveled.less_than_net(3)
    assert net.levels == 6 and net.entries == 5 and net.variables == 6 and net.widths[-1] == 1 and net.widths.max() <= 4
    for x in range(8):
        for y in range(8):
            bits = [(x >> b) & 1 for b in range(3)] + [(y >> b) & 1 for b in range(3)]
            assert net.evaluate_clear(table, bits) == [x < y], (x, y)


def test_tree_net_clear_equals_the_table_entry(tfhe):
    from tfhe_jl_amd import leveled
    net = leveled.tree_net(3)
    assert list(net.widths) == [4, 2, 1] and net.entries == 8 and net.variables == 3 and net.products == 7
    table = [10, 11, 12, 13, 14, 15, 16, 17]
    for address in range(8):
        assert net.evaluate_clear(table, [(address >> v) & 1 for v in range(3)]) == [table[address]]


def test_dfa_net_comparator_widths_and_copy_nodes(tfhe):
    from tfhe_jl_amd import leveled
    net = leveled.dfa_net([1, 0, 4, 3, 4], [2, 3, 0, 3, 4], 0, 8)
    assert list(net.widths) == [4, 3, 4, 3, 4, 3, 2, 1] and net.entries == 5 and net.variables == 8
    copies = net.nodes[net.nodes[:, 0] == net.nodes[:, 1]]
    assert len(copies) == 12 and net.products == 12                  # the two absorbing states wherever they are reachable
    assert net.level(0).tolist() == [[0, 3, 7], [4, 0, 7], [3, 3, 7], [4, 4, 7]]         # level 0 reads the table by state
    assert net.level(7).tolist() == [[0, 1, 0]]                                           # the start state reads letter 0
    lt, _ = leveled.less_than_net(4)
    assert list(lt.widths) == [4, 3, 4, 3, 4, 3, 2, 1]
    assert [int(r[2]) for r in (lt.level(v)[0] for v in range(8))] == [4, 0, 5, 1, 6, 2, 7, 3]      # y_0, x_0, y_1, ..., x_3


def test_cmux_net_rejects_what_the_library_rejects(tfhe):
    from tfhe_jl_amd import leveled
    ok = leveled.CmuxNet([2, 1], [[0, 1, 0], [1, 0, 1], [0, 1, 2]])
    assert ok.entries == 2 and ok.variables == 3 and ok.levels == 2
    with pytest.raises(ValueError, match="src1 = 2 is outside the 2 nodes below"):
        leveled.CmuxNet([2, 1], [[0, 1, 0], [1, 0, 1], [0, 2, 2]])                       # a source beyond the level below
    with pytest.raises(ValueError, match="src0 = 5 is outside the 5 table entries"):
        leveled.CmuxNet([1], [[5, 0, 0]], entries=5)
    with pytest.raises(ValueError):
        leveled.CmuxNet([2, 1], [[0, 1, 0], [1, 0, -1], [0, 1, 2]])                      # a negative var
    with pytest.raises(ValueError, match="var = 3"):
        leveled.CmuxNet([1], [[0, 1, 3]], variables=3)
    with pytest.raises(ValueError, match=r"widths\[1\] = 0"):
        leveled.CmuxNet([2, 0, 1], [[0, 1, 0], [1, 0, 1], [0, 1, 2]])                    # a zero width
    with pytest.raises(ValueError):
        leveled.CmuxNet([4097], np.zeros((4097, 3), np.int32))
    with pytest.raises(ValueError):
        leveled.CmuxNet([1] * 1025, np.zeros((1025, 3), np.int32))
    with pytest.raises(ValueError):
        leveled.CmuxNet([2, 1], [[0, 1, 0], [1, 0, 1]])                                  # a record short


def test_schoolbook_network_decrypts_the_comparator(tfhe):
    """N = 64, k = 1, l = 3, beta = 8, bs noise 1e-7: less_than_net(4) as a schoolbook network over tgsw_encrypt_bits selectors decrypts
    (tlwe_phase, coefficient 0) to x < y with the phase within 2^26 of +-2^29."""
    from tfhe_jl_amd import leveled
    N, k, l, beta, d = 64, 1, 3, 8, 4
    p = _params(tfhe, N, k, l, beta, bs_noise=1e-7)
    rng = np.random.default_rng(41)
    sk, ck = tfhe.make_key_pair(rng, p)
    net, table = leveled.less_than_net(d)
    data = leveled.table_to_tlwe(table, N, k)
    for x, y in [(5, 5), (5, 6), (5, 4), (0, 15), (15, 0), (9, 12)]:                      # x = y, y = x +- 1, the extremes, a mixed pair
        bits = [(x >> b) & 1 for b in range(d)] + [(y >> b) & 1 for b in range(d)]
        assert net.evaluate_clear(table, bits) == [x < y]
        tg = leveled.tgsw_encrypt_bits(rng, sk, bits)
        got = net_ref(Tree(N, k, l, beta, tg), net, data, list(range(2 * d)))
        assert got.shape == (1, k + 1, N)
        phase = leveled.tlwe_phase(sk, got[0].astype(np.int32))[0]
        assert (phase[0] > 0) == (x < y), (x, y, phase[0])
        assert abs(int(phase[0]) - (2**29 if x < y else -2**29)) < 2**26, (x, y, phase[0])
    ck.close()


# ---- 2. GPU: a random network word for word ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("N,k,l,beta", [(64, 1, 3, 8), (1024, 1, 2, 10), (1024, 2, 2, 10), (1024, 1, 4, 6)])
def test_gpu_random_network_equals_schoolbook(tfhe, N, k, l, beta):
    from tfhe_jl_amd import leveled
    B, T, E, V, S, widths = 3, 2, 5, 4, 6, [4, 3, 2]
    rng, sk, ck, eng, tgsw, tlwe = _setup(tfhe, N, k, l, beta, 6300 + N + k + l, S, T * E)
    data = tlwe.reshape(T, E, k + 1, N)
    net = leveled.CmuxNet(widths, random_net(rng, E, widths, V), entries=E, variables=V)
    assert net.products == 7
    sel = np.array([[0, 1, 2, 3], [5, 4, 0, 2], [3, 3, 1, 5]], np.int32)                  # rows differ; a selector behind two variables
    index = np.array([1, 0, 1], np.int32)
    want, want_ext = ref_rows(Tree(N, k, l, beta, tgsw), net, data, index, sel)
    eng.tgsw_load(tgsw)
    got0 = eng.cmux_net(data, net, sel, table_index=index, out_form=0)
    assert got0.shape == (B, 2, k + 1, N) and np.array_equal(got0, want), "out_form 0"
    assert eng.last_kernel_name() == f"cmux_net_level_kernel(N={N},k={k},l={l})"
    assert eng.last_rotation_count() == 0 and eng.last_timing_ms(0) > 0
    got1 = eng.cmux_net(data, net, sel, table_index=index, out_form=1)
    assert np.array_equal(got1, want_ext), "out_form 1"
    got2 = eng.cmux_net(data, net, sel, table_index=index, out_form=2)
    assert eng.last_timing_ms(1) > 0 and got2.shape == (B, 2, LWE + 1)
    assert np.array_equal(got2.reshape(B * 2, -1), eng.keyswitch(want_ext.reshape(B * 2, -1))), "out_form 2"
    from leveled_ref import ks_ref, ks_schoolbook                      # (imported here: leveled_ref imports, through test_rot_net, this module)
    assert np.array_equal(got2, ks_ref(ks_schoolbook(ck.params, ck.keyswitch_key), want_ext)), "out_form 2 against the integer keyswitch"
    # NULL table index = table 0 for every row
    want0, _ = ref_rows(Tree(N, k, l, beta, tgsw), net, data, [0] * B, sel[:1])
    assert np.array_equal(eng.cmux_net(data, net, sel[:1], out_form=0), want0)
    ck.close()


# ---- 3. GPU: a tree-shaped network is the CMUX tree -------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("N,k,l,beta", [(64, 1, 3, 8), (1024, 1, 2, 10)])
def test_gpu_tree_net_equals_cmux_tree(tfhe, N, k, l, beta):
    from tfhe_jl_amd import leveled
    B, T, depth = 3, 2, 3
    rng, sk, ck, eng, tgsw, tlwe = _setup(tfhe, N, k, l, beta, 6400 + N, 4, T * 8)
    data = tlwe.reshape(T, 8, k + 1, N)
    sel = rng.integers(0, 4, (B, depth)).astype(np.int32)
    index = np.array([1, 0, 1], np.int32)
    net = leveled.tree_net(depth)
    eng.tgsw_load(tgsw)
    for form in (0, 1, 2):
        tree = eng.cmux_tree(data, sel, table_index=index, out_form=form)
        got = eng.cmux_net(data, net, sel, table_index=index, out_form=form)
        assert got.shape == (B, 1) + tree.shape[1:] and np.array_equal(got[:, 0], tree), form
    ref = Tree(N, k, l, beta, tgsw)                                   # ... and both are the schoolbook's words, not each other's mistake
    assert np.array_equal(eng.cmux_net(data, net, sel[:1], table_index=index[:1], out_form=0)[0, 0], ref.tree(data[1], sel[0]).astype(np.int32))
    ck.close()


# ---- 4. GPU: workspaces sized by every level, regrown correctly -------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_workspace_parity_and_regrowth(tfhe):
    """Widths [2, 6, 3, 7, 1] as the first call of a fresh context (the odd levels are wider than level 0 and than every even level:
    buffers sized by level 0, or both by one maximum taken over the wrong parity, overflow or misplace rows), then a one-node network,
    then the first again."""
    from tfhe_jl_amd import leveled
    N, k, l, beta, B, E, V = 64, 1, 3, 8, 2, 3, 5
    rng, sk, ck, eng, tgsw, tlwe = _setup(tfhe, N, k, l, beta, 6500, 5, E)
    data = tlwe.reshape(1, E, k + 1, N)
    widths = [2, 6, 3, 7, 1]
    nodes = []
    for v, w in enumerate(widths):
        below = E if v == 0 else widths[v - 1]
        nodes += [[i % below, (i + 1 + v) % below if below > 1 else 0, (i + v) % V] for i in range(w)]
    big = leveled.CmuxNet(widths, nodes, entries=E, variables=V)
    one = leveled.CmuxNet([1], [[2, 0, 4]], entries=E, variables=V)
    sel = np.array([[0, 1, 2, 3, 4], [4, 2, 0, 1, 3]], np.int32)
    ref = Tree(N, k, l, beta, tgsw)
    eng.tgsw_load(tgsw)
    for net in (big, one, big):
        want, want_ext = ref_rows(ref, net, data, [0] * B, sel)
        assert np.array_equal(eng.cmux_net(data, net, sel, out_form=0), want), list(net.widths)
        assert np.array_equal(eng.cmux_net(data, net, sel, out_form=1), want_ext), list(net.widths)
    ck.close()


# ---- 5. GPU: spectrum accumulators in global memory -------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_accumulators_in_global_memory_small(tfhe):
    from tfhe_jl_amd import leveled
    N, k, l, beta, E, V, widths = 64, 1, 3, 8, 5, 4, [4, 3, 2]
    rng, sk, ck, eng, tgsw, tlwe = _setup(tfhe, N, k, l, beta, 6600, 6, E)
    net = leveled.CmuxNet(widths, random_net(rng, E, widths, V), entries=E, variables=V)
    sel = np.array([[0, 1, 2, 3], [5, 4, 0, 2]], np.int32)
    eng.tgsw_load(tgsw)
    lds = [eng.cmux_net(tlwe, net, sel, out_form=f) for f in (0, 1, 2)]
    assert eng.last_kernel_name() == f"cmux_net_level_kernel(N={N},k={k},l={l})"
    eng.set_option("anyn_spec", 1)
    glob = [eng.cmux_net(tlwe, net, sel, out_form=f) for f in (0, 1, 2)]
    assert eng.last_kernel_name().endswith(",spec=global)") and eng.last_kernel_name().startswith("cmux_net_level_kernel(")
    for a, b in zip(lds, glob):
        assert np.array_equal(a, b)
    want, _ = ref_rows(Tree(N, k, l, beta, tgsw), net, tlwe[None], [0, 0], sel)
    assert np.array_equal(glob[0], want)
    ck.close()


@pytest.mark.gpu
def test_gpu_accumulators_in_global_memory_n8192(tfhe):
    """N = 8192, k = 1, l = 2, beta = 7: three spectra of 4608 complex words exceed 160 KB of LDS, so the accumulators can only live in
    global memory; widths [2, 1], one row, against the schoolbook."""
    from tfhe_jl_amd import leveled
    N, k, l, beta = 8192, 1, 2, 7
    rng, sk, ck, eng, tgsw, tlwe = _setup(tfhe, N, k, l, beta, 6700, 2, 3)
    net = leveled.CmuxNet([2, 1], [[0, 1, 0], [2, 1, 1], [1, 0, 1]], entries=3, variables=2)
    sel = np.array([[1, 0]], np.int32)
    eng.tgsw_load(tgsw)
    got = eng.cmux_net(tlwe, net, sel, out_form=0)
    assert eng.last_kernel_name() == f"cmux_net_level_kernel(N={N},k={k},l={l},spec=global)"
    want, _ = ref_rows(Tree(N, k, l, beta, tgsw), net, tlwe[None], [0], sel)
    assert np.array_equal(got, want)
    ck.close()


# ---- 6. GPU: the comparator at full size ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_less_than_16_bits_full_size(tfhe, keys80):
    """less_than_net(16) under tfhe_parameters_80, 8 pairs, out_form 2: all 8 decrypt to x < y and their gate_not to the opposite."""
    from tfhe_jl_amd import leveled
    K, d = keys80, 16
    p = K.params
    N, k, l = p.tlwe_polynomial_degree, p.tlwe_mask_size, p.bs_decomp_length
    rng = np.random.default_rng(8816)
    net, table = leveled.less_than_net(d)
    assert net.levels == 32 and net.widths.max() == 4
    pairs = [(12345, 12345), (40000, 40000 ^ 1), (40001, 40001 ^ 1), (0, 65535), (65535, 0), (0x8000, 0x7FFF)]
    pairs += [tuple(int(v) for v in rng.integers(0, 65536, 2)) for _ in range(2)]
    bits = np.array([[(x >> b) & 1 for b in range(d)] + [(y >> b) & 1 for b in range(d)] for x, y in pairs])
    tgsw = leveled.tgsw_encrypt_bits(rng, K.sk, bits.reshape(-1)).reshape(len(pairs), 2 * d, l, k + 1, k + 1, N)
    out = leveled.cmux_net_lookup(K.ck, leveled.table_to_tlwe(table, N, k), net, tgsw)
    want = np.array([x < y for x, y in pairs])
    assert len(out) == 8 and np.array_equal(tfhe.decrypt(K.sk, out), want)
    assert np.array_equal(tfhe.decrypt(K.sk, tfhe.gate_not(K.ck, out)), ~want)


# ---- 7. GPU: the contract ---------------------------------------------------------------------------------------------------------
def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class _Call:
    """A valid raw call of tfhe_cmux_net_batch whose arguments can be replaced one at a time."""

    def __init__(self, eng, data, net, sel):
        self.eng, self.F = eng, int(net.widths[-1])
        self.base = dict(data=data, T=data.shape[0], E=data.shape[1], table_index=None, widths=net.widths, levels=net.levels, nodes=net.nodes,
                         sel=sel, V=sel.shape[1], B=sel.shape[0], out_form=0)

    def __call__(self, **over):
        a = dict(self.base, **over)
        out = np.zeros((self.base["B"], self.F) + self.base["data"].shape[2:], np.int32)
        rc = self.eng._lib.tfhe_cmux_net_batch(self.eng._h, _ptr(a["data"]), a["T"], a["E"], _ptr(a["table_index"]), _ptr(a["widths"]), a["levels"],
                                               _ptr(a["nodes"]), _ptr(a["sel"]), a["V"], _ptr(out), a["B"], a["out_form"])
        return rc, self.eng._lib.tfhe_last_error(self.eng._h).decode(), out


def _mem_free():
    hip = C.CDLL("libamdhip64.so")
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0 and 0 < free.value <= total.value
    return free.value


@pytest.mark.gpu
def test_gpu_contract_refusals_leave_the_context_usable(tfhe):
    from tfhe_jl_amd import leveled
    N, k, l, beta, E, V, S = 64, 1, 3, 8, 3, 2, 3
    p = _params(tfhe, N, k, l, beta, n=16, bs_noise=1e-7)
    rng = np.random.default_rng(97)
    sk, ck = tfhe.make_key_pair(rng, p)
    eng = ck.engine(0)
    tg = leveled.tgsw_encrypt_bits(rng, sk, [1, 0, 1])
    data = leveled.tlwe_encrypt(rng, sk, _words(rng, E, N))[None]
    net = leveled.CmuxNet([2, 1], [[0, 1, 0], [2, 1, 1], [1, 0, 1]], entries=E, variables=V)
    sel = np.array([[0, 1], [2, 0]], np.int32)
    want, want_ext = ref_rows(Tree(N, k, l, beta, tg), net, data, [0, 0], sel)
    call = _Call(eng, data, net, sel)

    def still_right():
        rc, msg, out = call()
        assert rc == 0 and np.array_equal(out, want), msg

    def refused(code, word, **over):
        rc, msg, _ = call(**over)
        assert rc == code and word in msg and "cmux_net_batch" in msg, (over.keys(), rc, msg)
        still_right()

    rc, msg, _ = call()
    assert rc == NO_KEY and "selector" in msg                          # no selector set yet
    eng.tgsw_load(tg)
    still_right()
    for name in ("data", "widths", "nodes", "sel"):
        refused(INVALID, "NULL", **{name: None})
    for levels in (0, -1, 1025, 4096):
        refused(INVALID, "levels", levels=levels)
    for w in (0, 4097, -3):
        refused(INVALID, "widths[1]", widths=np.array([2, w], np.int32))
    refused(INVALID, "E =", E=0)
    refused(INVALID, "V =", V=0)
    refused(INVALID, "T =", T=0)
    bad = net.nodes.copy(); bad[1, 0] = 3                              # level 0: a source past the table
    refused(INVALID, "src0 = 3", nodes=bad)
    bad = net.nodes.copy(); bad[2, 1] = 2                              # level 1: a source past the two nodes below
    refused(INVALID, "src1 = 2", nodes=bad)
    bad = net.nodes.copy(); bad[0, 0] = -1
    refused(INVALID, "src0 = -1", nodes=bad)
    for var in (V, -1):
        bad = net.nodes.copy(); bad[2, 2] = var
        refused(INVALID, f"var = {var}", nodes=bad)
    for s in (S, -1):
        bad = sel.copy(); bad[1, 0] = s
        refused(INVALID, "sel[1][0]", sel=bad)
    for t in (1, -1):
        refused(INVALID, "table_index[1]", table_index=np.array([0, t], np.int32))
    for form in (3, -1):
        refused(INVALID, "out_form", out_form=form)
    refused(INVALID, "exceed one launch", B=2**30)                     # B * widths[0] = 2^31 (refused before sel is read)
    rc, msg, _ = call(B=0, data=None, sel=None)
    assert rc == 0
    eng.set_option("measure_margin", 1)
    refused_rc, msg, _ = call()
    assert refused_rc == STATE and "measure_margin" in msg
    eng.set_option("measure_margin", 0)
    still_right()
    # out_form 2 without the keyswitch key; forms 0 and 1 do not need it
    raw = tfhe.Engine(p)
    raw.load_bootstrap_key(ck.bootstrap_key)
    raw.tgsw_load(tg)
    with pytest.raises(tfhe.EngineError) as e:
        raw.cmux_net(data, net, sel, out_form=2)
    assert e.value.code == NO_KEY
    assert np.array_equal(raw.cmux_net(data, net, sel, out_form=1), want_ext)
    raw.load_keyswitch_key(ck.keyswitch_key)
    assert np.array_equal(raw.cmux_net(data, net, sel), eng.cmux_net(data, net, sel))
    assert np.array_equal(eng.cmux_net(data, net, sel).reshape(2, -1), eng.keyswitch(want_ext.reshape(2, -1)))
    raw.close()
    # a multi-device context
    multi = ck.engine([0, 0])
    with pytest.raises(tfhe.EngineError) as e:
        multi.cmux_net(data, net, sel)
    assert e.value.code == STATE
    bx = tfhe.encrypt(rng, sk, [True, False]).data
    assert np.array_equal(tfhe.decrypt(sk, multi.gates(np.zeros(2, np.uint8), bx, bx)), [False, True])
    # an injected allocation failure through the new entry point: NOMEM, and the context goes on working
    lib = eng._lib
    assert lib.tfhe_set_option(None, b"debug_fail_alloc_after", 1) == 0
    rc, msg, _ = call()
    lib.tfhe_set_option(None, b"debug_fail_alloc_after", 0)
    assert rc == NOMEM and "memory" in msg, (rc, msg)
    still_right()
    ck.close()


@pytest.mark.gpu
def test_gpu_multikey_context_refuses_cmux_net(tfhe):
    from test_independent import _mk_setup
    from tfhe_jl_amd import leveled
    p, sks, ck, xs, ys, want = _mk_setup(tfhe, 2, 4, 7, 3, 402)
    eng = ck.engine(0)
    net = leveled.CmuxNet([1], [[0, 1, 0]])
    with pytest.raises(tfhe.EngineError) as e:
        eng.cmux_net(np.zeros((2, 2, 1024), np.int32), net, np.zeros((1, 1), np.int32))
    assert e.value.code == STATE and "multi-key" in str(e.value)
    assert np.array_equal(eng.mk_gate_nand(xs, ys), want)            # the context still runs its own gates
    ck.close()


@pytest.mark.gpu
def test_gpu_oversized_network_is_refused_before_allocating(tfhe):
    """1024 levels of 4096 nodes at B = 2^19 - 1 rows: one workspace alone is 1.1 TB.  TFHE_ERR_NOMEM, computed and refused before any
    allocation (hipMemGetInfo reads unchanged), and the context goes on working."""
    from tfhe_jl_amd import leveled
    N, k, l, beta = 64, 1, 3, 8
    p = _params(tfhe, N, k, l, beta, n=16, bs_noise=1e-7)
    rng = np.random.default_rng(13)
    sk, ck = tfhe.make_key_pair(rng, p)
    eng = ck.engine(0)
    eng.tgsw_load(leveled.tgsw_encrypt_bits(rng, sk, [1]))
    table = leveled.table_to_tlwe([True, False], N, k)
    small = leveled.CmuxNet([1], [[1, 0, 0]])                         # selector bit 1 picks src1 = entry 0
    assert list(tfhe.decrypt(sk, eng.cmux_net(table, small, np.zeros((1, 1), np.int32))[:, 0])) == [True]
    B = 2**19 - 1
    huge = leveled.CmuxNet([4096] * 1024, np.zeros((4096 * 1024, 3), np.int32), entries=2, variables=1)
    sel = np.zeros((B, 1), np.int32)
    before = _mem_free()
    rc = eng._lib.tfhe_cmux_net_batch(eng._h, _ptr(table), 1, 2, None, _ptr(huge.widths), huge.levels, _ptr(huge.nodes), _ptr(sel), 1,
                                      _ptr(np.zeros(1, np.int32)), B, 0)
    assert rc == NOMEM and "MB" in eng._lib.tfhe_last_error(eng._h).decode()
    assert _mem_free() == before
    assert list(tfhe.decrypt(sk, eng.cmux_net(table, small, np.zeros((1, 1), np.int32))[:, 0])) == [True]
    ck.close()
