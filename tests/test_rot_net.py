"""CMUX networks with monomial edges (tfhe_rot_net_batch; tfhe_jl_amd.leveled.RotNet, pack_table_to_tlwe, packed_lookup_net, wfa_net)
against an integer schoolbook network.

The reference of every word comparison is `rot_net_ref` below: tests/test_leveled.py's `Tree.cmux` (exact int64, np.convolve, no
transform, no rounding) per node on sources rotated by tests/test_independent.py's `monomial` (X^s p, coefficient by coefficient), a
rotated copy copying the rotated words — never the engine.  Operands come from test_leveled's `_setup`: arbitrary Int32 words with the
extreme rows where the set is exact for any words (exact_domain 2), real encryptions elsewhere.

Noise (why "all 8 addresses correct" at full size is a condition, not a measurement): a packed lookup of a 4096-entry table at
tfhe_parameters_80 is 3 tree levels and 10 rotation levels, 13 external products on the path, each adding one product's noise (3e-4 of
the torus, tests/test_leveled.py) to a window of 1/8; a rotation by a public monomial permutes and negates coefficients and adds
nothing.  The schoolbook network alone gave 8 of 8 for exactly the addresses of the full-size test, with the worst phase error 2.2e-3
of the torus, 55 times inside the window.  At N = 64, l = 3, beta = 8, bs noise 1e-7 and depth 8 (2 tree levels, 6 rotation levels)
the schoolbook decrypts 256 of 256 addresses with the worst phase error 1.25e-3 of the torus; the bound asserted there is 2^26 / 2^32
= 1.6e-2.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from test_cmux_net import random_net
from test_independent import monomial, wrap32
from test_leveled import LWE_N as LWE, Tree, _params, _setup, _words

INVALID, NO_KEY, STATE, NOMEM = 1, 3, 5, 6


def rot(sample, r, N):
    """X^r on every polynomial of a sample [k+1][N] (mask and body), wrapped to 32-bit words: -(-2^31) stays -2^31."""
    return wrap32(np.stack([monomial(p, int(r), N) for p in np.asarray(sample, np.int64)]))


def rot_net_ref(ref, net, table, sels):
    """The schoolbook network: `ref` a Tree over the selector set, `table` [E][k+1][N], sels[var] the selector behind each variable of
    the row.  Returns the outputs of the last level, int64 [F][k+1][N]."""
    N = net.degree
    cur = [np.asarray(t, np.int64) for t in table]
    for v in range(net.levels):
        nxt = []
        for s0, s1, var, r0, r1 in net.level(v).tolist():
            a = rot(cur[s0], r0, N)
            nxt.append(a if (s0, r0) == (s1, r1) else ref.cmux(sels[var], a, rot(cur[s1], r1, N)))
        cur = nxt
    return np.stack(cur)


def ref_rows(ref, net, data, rows, sel):
    want = np.stack([rot_net_ref(ref, net, data[rows[g]], sel[g]) for g in range(len(sel))])             # [B][F][k+1][N]
    ext = np.stack([[ref.extract(w) for w in row] for row in want]).astype(np.int32)                      # [B][F][kN+1]
    return want.astype(np.int32), ext


def random_rot_net(leveled, rng, N, E, V):
    """test_cmux_net's random_net at widths [4, 3, 2] (a copy at level 0 and one at the last level, a node with src0 > src1) with random
    rotations and, planted: the values 0, 1, M, N - 1, N, N + 1, 2N - 1; both copies rotated (1 at level 0; N + 1 at the last level: the
    extraction of a rotated, negated copy); a node with src0 == src1 and rot0 != rot1 (a true product).  7 products."""
    widths = [4, 3, 2]
    nodes = [rec + [int(r) for r in rng.integers(0, 2 * N, 2)] for rec in random_net(rng, E, widths, V)]
    nodes[0][3:] = [1, 1]                                             # the rotated copy of level 0
    nodes[1][3:] = [0, 2 * N - 1]                                     # src0 > src1
    nodes[2][3:] = [N // 2, N]
    nodes[3][3:] = [N - 1, N + 1]
    nodes[4][1] = nodes[4][0]
    nodes[4][3:] = [0, N]                                             # one source, two rotations: a product
    nodes[-1][3:] = [N + 1, N + 1]                                    # the rotated copy of the last level
    net = leveled.RotNet(widths, nodes, N, entries=E, variables=V)
    assert net.products == 7
    return net


def packed_plain(values, N):
    """pack_table_to_tlwe's layout on plain integer polynomials: entry i on coefficient i & (2^r - 1) of polynomial i >> r."""
    r = min(len(values).bit_length() - 1, N.bit_length() - 1)
    out = np.zeros((len(values) >> r, N), np.int64)
    out[:, :1 << r] = np.asarray(values, np.int64).reshape(-1, 1 << r)
    return out


# ---- 1. CPU: the builders, the validation, the reference itself -------------------------------------------------------------------
@pytest.mark.parametrize("d,N,r,E", [(5, 8, 3, 4), (3, 8, 3, 1)])
def test_packed_lookup_net_clear_returns_the_entry_at_coefficient_0(tfhe, d, N, r, E):
    from tfhe_jl_amd import leveled
    net = leveled.packed_lookup_net(d, N)
    assert net.entries == E and net.variables == d and net.levels == d and net.products == E - 1 + r
    assert net.level(d - r).tolist() == [[0, 0, 0, 0, 2 * N - 1]] and net.level(d - 1).tolist() == [[0, 0, r - 1, 0, 2 * N - (1 << (r - 1))]]
    values = [100 + 7 * i for i in range(1 << d)]
    table = packed_plain(values, N)
    assert table.shape == (E, N)
    for address in range(1 << d):
        out = net.evaluate_clear(table, [(address >> v) & 1 for v in range(d)])
        assert len(out) == 1 and out[0].shape == (N,) and out[0][0] == values[address], address
    # ... and the packed TLWE table is that layout, encoded, on the body of trivial samples
    tl = leveled.pack_table_to_tlwe(values, N, k=1, encode=lambda v: v)
    assert tl.shape == (E, 2, N) and tl.dtype == np.int32 and not tl[:, 0].any() and np.array_equal(tl[:, 1], table)
    small = leveled.pack_table_to_tlwe([3, 4], N, encode=lambda v: v)                    # r = depth < log2 N: the rest is zero
    assert small.shape == (1, 2, N) and small[0, 1].tolist() == [3, 4] + [0] * (N - 2)


def test_wfa_net_popcount_over_six_bits(tfhe):
    """One state, weights 0 and 2N - 1 (X^-1 per set letter): the output is X^(-popcount) tv, tv[popcount] at coefficient 0."""
    from tfhe_jl_amd import leveled
    N, steps = 8, 6
    net = leveled.wfa_net([0], [0], [0], [2 * N - 1], 0, steps, N)
    assert list(net.widths) == [1] * steps and net.entries == 1 and net.variables == steps and net.products == steps
    assert net.level(0).tolist() == [[0, 0, steps - 1, 0, 2 * N - 1]]
    tv = np.array([50 + 3 * c for c in range(N)])
    for x in range(1 << steps):
        bits = [(x >> b) & 1 for b in range(steps)]
        assert net.evaluate_clear([tv], bits)[0][0] == tv[sum(bits)], x
    # weights are taken mod 2N; a state whose two transitions and weights agree is a rotated copy
    same = leveled.wfa_net([0], [0], [-1], [2 * N - 1], 0, 2, N)
    assert same.nodes.tolist() == [[0, 0, 1, 2 * N - 1, 2 * N - 1], [0, 0, 0, 2 * N - 1, 2 * N - 1]] and same.products == 0
    assert same.evaluate_clear([tv], [0, 1])[0].tolist() == monomial(monomial(tv, -1, N), -1, N).tolist()


def test_rot_net_rejects_what_the_library_rejects(tfhe):
    from tfhe_jl_amd import leveled
    N = 8
    ok = leveled.RotNet([2, 1], [[0, 1, 0, 0, 15], [1, 0, 1, 8, 8], [0, 1, 2, 3, 3]], N)
    assert ok.entries == 2 and ok.variables == 3 and ok.levels == 2 and ok.degree == N and ok.products == 3
    assert ok.level(1).tolist() == [[0, 1, 2, 3, 3]]
    with pytest.raises(ValueError, match=r"node 1 of level 0: rot0 = -1 is outside \[0, 16\)"):
        leveled.RotNet([2, 1], [[0, 1, 0, 0, 15], [1, 0, 1, -1, 8], [0, 1, 2, 3, 3]], N)
    with pytest.raises(ValueError, match=r"node 0 of level 1: rot1 = 16 is outside \[0, 16\)"):
        leveled.RotNet([2, 1], [[0, 1, 0, 0, 15], [1, 0, 1, 8, 8], [0, 1, 2, 3, 16]], N)
    with pytest.raises(ValueError, match=r"\[3\]\[5\] = \(src0, src1, var, rot0, rot1\)"):
        leveled.RotNet([2, 1], [[0, 1, 0, 0], [1, 0, 1, 8], [0, 1, 2, 3]], N)           # a four-word record
    with pytest.raises(ValueError, match="node 0 of level 1: src1 = 2 is outside the 2 nodes below"):
        leveled.RotNet([2, 1], [[0, 1, 0, 0, 0], [1, 0, 1, 0, 0], [0, 2, 2, 0, 0]], N)
    with pytest.raises(ValueError, match="node 0 of level 0: var = 3"):
        leveled.RotNet([1], [[0, 1, 3, 0, 0]], N, variables=3)
    with pytest.raises(ValueError, match=r"widths\[1\] = 0"):
        leveled.RotNet([2, 0, 1], np.zeros((3, 5), np.int32), N)
    with pytest.raises(ValueError, match="degree"):
        leveled.RotNet([1], [[0, 1, 0, 0, 0]], 12)
    for depth, n in ((0, 8), (25, 1 << 13), (16, 8)):                                     # 2^13 table samples at (16, 8)
        with pytest.raises(ValueError, match="depth"):
            leveled.packed_lookup_net(depth, n)
    assert leveled.packed_lookup_net(16, 1024).products == 63 + 10 and leveled.packed_lookup_net(8, 1024).products == 8


@functools.lru_cache(maxsize=None)
def _packed_case(tfhe):
    """N = 64, k = 1, l = 3, beta = 8, bs noise 1e-7, depth 8: an encrypted packed table of 256 random bits (E = 4 samples), 16 selectors
    (selector 2 v + bit encrypts `bit`, the one behind variable v of an address whose bit v is `bit`) and the schoolbook network's
    output for every address, computed once for the CPU and the GPU test."""
    from tfhe_jl_amd import leveled
    N, k, l, beta, d = 64, 1, 3, 8, 8
    p = _params(tfhe, N, k, l, beta, bs_noise=1e-7)
    rng = np.random.default_rng(4141)
    sk, ck = tfhe.make_key_pair(rng, p)
    bits = rng.integers(0, 2, 1 << d).astype(bool)
    data = leveled.pack_table_to_tlwe(bits, N, k, rng=rng, secret_key=sk)
    tgsw = leveled.tgsw_encrypt_bits(rng, sk, [0, 1] * d)
    net = leveled.packed_lookup_net(d, N)
    sel = np.array([[2 * v + ((a >> v) & 1) for v in range(d)] for a in range(1 << d)], np.int32)
    want, want_ext = ref_rows(Tree(N, k, l, beta, tgsw), net, data[None], [0] * len(sel), sel)
    return sk, ck, bits, data, tgsw, net, sel, want, want_ext


def test_schoolbook_packed_lookup_decrypts_every_address(tfhe):
    """The schoolbook network of packed_lookup_net(8, 64) (2 tree levels, then 6 rotation levels) over tgsw_encrypt_bits selectors
    decrypts (tlwe_phase, coefficient 0) to table[address] for all 256 addresses, the phase within 2^26 of +-2^29."""
    from tfhe_jl_amd import leveled
    sk, ck, bits, data, tgsw, net, sel, want, want_ext = _packed_case(tfhe)
    assert data.shape == (4, 2, 64) and list(net.widths) == [2, 1] + [1] * 6 and net.products == 9
    phase = leveled.tlwe_phase(sk, want[:, 0])[:, 0].astype(np.int64)                   # [256] coefficient 0 of every row's output
    target = np.where(bits, 2**29, -2**29)
    print("worst phase error:", np.abs(phase - target).max() / 2**32, "of the torus")
    assert np.array_equal(phase > 0, bits)
    assert np.abs(phase - target).max() < 2**26


# ---- 2. GPU: a random network word for word ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("N,k,l,beta", [(64, 1, 3, 8), (1024, 1, 2, 10), (1024, 2, 2, 10), (1024, 1, 4, 6)])
def test_gpu_random_network_equals_schoolbook(tfhe, N, k, l, beta):
    from tfhe_jl_amd import leveled
    B, T, E, V, S = 3, 2, 5, 4, 6
    rng, sk, ck, eng, tgsw, tlwe = _setup(tfhe, N, k, l, beta, 7300 + N + k + l, S, T * E)
    data = tlwe.reshape(T, E, k + 1, N)
    net = random_rot_net(leveled, rng, N, E, V)
    sel = np.array([[0, 1, 2, 3], [5, 4, 0, 2], [3, 3, 1, 5]], np.int32)                  # rows differ; a selector behind two variables
    index = np.array([1, 0, 1], np.int32)
    want, want_ext = ref_rows(Tree(N, k, l, beta, tgsw), net, data, index, sel)
    eng.tgsw_load(tgsw)
    got0 = eng.rot_net(data, net, sel, table_index=index, out_form=0)
    assert got0.shape == (B, 2, k + 1, N) and np.array_equal(got0, want), "out_form 0"
    assert eng.last_kernel_name() == f"rot_net_level_kernel(N={N},k={k},l={l})"
    assert eng.last_rotation_count() == 0 and eng.last_timing_ms(0) > 0
    got1 = eng.rot_net(data, net, sel, table_index=index, out_form=1)
    assert np.array_equal(got1, want_ext), "out_form 1"
    got2 = eng.rot_net(data, net, sel, table_index=index, out_form=2)
    assert eng.last_timing_ms(1) > 0 and got2.shape == (B, 2, LWE + 1)
    assert np.array_equal(got2.reshape(B * 2, -1), eng.keyswitch(want_ext.reshape(B * 2, -1))), "out_form 2"
    from leveled_ref import ks_ref, ks_schoolbook                      # (imported here: leveled_ref imports rot_net_ref from this module)
    assert np.array_equal(got2, ks_ref(ks_schoolbook(ck.params, ck.keyswitch_key), want_ext)), "out_form 2 against the integer keyswitch"
    # NULL table index = table 0 for every row
    want0, _ = ref_rows(Tree(N, k, l, beta, tgsw), net, data, [0], sel[:1])
    assert np.array_equal(eng.rot_net(data, net, sel[:1], out_form=0), want0)
    ck.close()


# ---- 3. GPU: rotated copies never pass through floating point ---------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_rotated_copies_on_arbitrary_words(tfhe):
    """A network of rotated copies only, two levels deep, on arbitrary Int32 tables with all-(-2^31), all-(2^31 - 1) and all-zero
    samples: the exact words of the host's rotation (the negation of -2^31 is -2^31), as samples and extracted."""
    from tfhe_jl_amd import leveled
    N, k, l, beta, E = 64, 1, 3, 8, 5
    rng, sk, ck, eng, tgsw, _ = _setup(tfhe, N, k, l, beta, 7400, 2, 3)
    data = _words(rng, 2, E, k + 1, N)
    data[0, 0], data[0, 1], data[0, 2] = -2**31, 2**31 - 1, 0
    data[1, 4, 0], data[1, 4, 1, ::2] = -2**31, -2**31
    rots = [1, N, 2 * N - 1]
    level0 = [[e, e, 0, rots[e % 3], rots[e % 3]] for e in range(E)] + [[0, 0, 0, N, N]]
    level1 = [[i, i, 0, rots[(i + 1) % 3], rots[(i + 1) % 3]] for i in (5, 0, 1, 4)]
    net = leveled.RotNet([6, 4], level0 + level1, N, entries=E, variables=1)
    assert net.products == 0
    index = np.array([0, 1, 0], np.int32)
    sel = np.zeros((3, 1), np.int32)
    want, want_ext = ref_rows(Tree(N, k, l, beta, tgsw), net, data, index, sel)
    assert np.array_equal(want[0, 0], np.full((k + 1, N), -2**31))                       # X^N X^N (-2^31 ...) in 32-bit words
    eng.tgsw_load(tgsw)
    assert np.array_equal(eng.rot_net(data, net, sel, table_index=index, out_form=0), want)
    assert np.array_equal(eng.rot_net(data, net, sel, table_index=index, out_form=1), want_ext)
    ck.close()


# ---- 4. GPU: with every rotation 0 the network is tfhe_cmux_net_batch --------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("N,k,l,beta", [(64, 1, 3, 8), (1024, 1, 2, 10)])
def test_gpu_zero_rotations_equal_cmux_net(tfhe, N, k, l, beta):
    from tfhe_jl_amd import leveled
    B, T, E, V, widths = 3, 2, 5, 4, [4, 3, 2]
    rng, sk, ck, eng, tgsw, tlwe = _setup(tfhe, N, k, l, beta, 7500 + N, 6, T * E)
    data = tlwe.reshape(T, E, k + 1, N)
    plain = leveled.CmuxNet(widths, random_net(rng, E, widths, V), entries=E, variables=V)
    net = leveled.RotNet(widths, np.concatenate([plain.nodes, np.zeros((9, 2), np.int32)], axis=1), N, entries=E, variables=V)
    sel = np.array([[0, 1, 2, 3], [5, 4, 0, 2], [3, 3, 1, 5]], np.int32)
    index = np.array([1, 0, 1], np.int32)
    eng.tgsw_load(tgsw)
    for form in (0, 1, 2):
        a = eng.cmux_net(data, plain, sel, table_index=index, out_form=form)
        b = eng.rot_net(data, net, sel, table_index=index, out_form=form)
        assert a.shape == b.shape and np.array_equal(a, b), form
    want, _ = ref_rows(Tree(N, k, l, beta, tgsw), net, data, index[:1], sel[:1])          # ... and both are the schoolbook's words
    assert np.array_equal(eng.rot_net(data, net, sel[:1], table_index=index[:1], out_form=0), want)
    ck.close()


# ---- 5. GPU: the kernel's rotation is the host's -----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_rotation_commutes_with_the_host(tfhe):
    """One level of rotated nodes equals tfhe_cmux_net_batch on a table the host rotated with `monomial`: entry 2i is X^rot0 in[src0] of
    node i, entry 2i + 1 is X^rot1 in[src1]."""
    from tfhe_jl_amd import leveled
    N, k, l, beta, E, V = 1024, 1, 2, 10, 4, 2
    rng, sk, ck, eng, tgsw, tlwe = _setup(tfhe, N, k, l, beta, 7600, 3, E)
    nodes = [[0, 1, 0, 1, 2 * N - 1], [3, 2, 1, N, N - 1], [1, 1, 0, 0, N + 1], [2, 0, 1, N // 2, 0], [2, 2, 1, 5, 5]]
    net = leveled.RotNet([5], nodes, N, entries=E, variables=V)
    rotated = np.stack([rot(tlwe[s], r, N) for s0, s1, var, r0, r1 in nodes for s, r in ((s0, r0), (s1, r1))]).astype(np.int32)
    plain = leveled.CmuxNet([5], [[2 * i, 2 * i + 1, nodes[i][2]] for i in range(4)] + [[8, 8, 1]], entries=10, variables=V)
    sel = np.array([[0, 1], [2, 0]], np.int32)
    eng.tgsw_load(tgsw)
    for form in (0, 1):
        assert np.array_equal(eng.rot_net(tlwe, net, sel, out_form=form), eng.cmux_net(rotated, plain, sel, out_form=form)), form
    ck.close()


# ---- 6. GPU: a packed lookup at every address --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_packed_lookup_every_address(tfhe):
    """packed_lookup_net(8, 64) at B = 256, one row per address, word for word against the schoolbook of the CPU test above."""
    sk, ck, bits, data, tgsw, net, sel, want, want_ext = _packed_case(tfhe)
    eng = ck.engine(0)
    eng.tgsw_load(tgsw)
    got = eng.rot_net(data, net, sel, out_form=0)
    assert got.shape == (256, 1, 2, 64) and np.array_equal(got, want)
    assert np.array_equal(eng.rot_net(data, net, sel, out_form=1), want_ext)
    ck.close()


# ---- 7. GPU: workspaces sized by every level, regrown correctly -------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_workspace_parity_and_regrowth(tfhe):
    """Widths [2, 6, 3, 7, 1] as the first call of a fresh context (the odd levels are wider than level 0 and than every even level),
    then a one-node network, then the first again, all with non-zero rotations."""
    from tfhe_jl_amd import leveled
    N, k, l, beta, B, E, V = 64, 1, 3, 8, 2, 3, 5
    rng, sk, ck, eng, tgsw, tlwe = _setup(tfhe, N, k, l, beta, 7700, 5, E)
    data = tlwe.reshape(1, E, k + 1, N)
    widths = [2, 6, 3, 7, 1]
    nodes = []
    for v, w in enumerate(widths):
        below = E if v == 0 else widths[v - 1]
        nodes += [[i % below, (i + 1 + v) % below if below > 1 else 0, (i + v) % V, 1 + (37 * i + 11 * v) % (2 * N - 1), 1 + (53 * i + 29 * v) % (2 * N - 1)]
                  for i in range(w)]
    big = leveled.RotNet(widths, nodes, N, entries=E, variables=V)
    one = leveled.RotNet([1], [[2, 0, 4, N + 3, 7]], N, entries=E, variables=V)
    sel = np.array([[0, 1, 2, 3, 4], [4, 2, 0, 1, 3]], np.int32)
    ref = Tree(N, k, l, beta, tgsw)
    eng.tgsw_load(tgsw)
    for net in (big, one, big):
        want, want_ext = ref_rows(ref, net, data, [0] * B, sel)
        assert np.array_equal(eng.rot_net(data, net, sel, out_form=0), want), list(net.widths)
        assert np.array_equal(eng.rot_net(data, net, sel, out_form=1), want_ext), list(net.widths)
    ck.close()


# ---- 8. GPU: spectrum accumulators in global memory -------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_accumulators_in_global_memory_small(tfhe):
    from tfhe_jl_amd import leveled
    N, k, l, beta, E, V = 64, 1, 3, 8, 5, 4
    rng, sk, ck, eng, tgsw, tlwe = _setup(tfhe, N, k, l, beta, 7800, 6, E)
    net = random_rot_net(leveled, rng, N, E, V)
    sel = np.array([[0, 1, 2, 3], [5, 4, 0, 2]], np.int32)
    eng.tgsw_load(tgsw)
    lds = [eng.rot_net(tlwe, net, sel, out_form=f) for f in (0, 1, 2)]
    assert eng.last_kernel_name() == f"rot_net_level_kernel(N={N},k={k},l={l})"
    eng.set_option("anyn_spec", 1)
    glob = [eng.rot_net(tlwe, net, sel, out_form=f) for f in (0, 1, 2)]
    assert eng.last_kernel_name() == f"rot_net_level_kernel(N={N},k={k},l={l},spec=global)"
    for a, b in zip(lds, glob):
        assert np.array_equal(a, b)
    want, _ = ref_rows(Tree(N, k, l, beta, tgsw), net, tlwe[None], [0, 0], sel)
    assert np.array_equal(glob[0], want)
    ck.close()


@pytest.mark.gpu
def test_gpu_accumulators_in_global_memory_n8192(tfhe):
    """N = 8192, k = 1, l = 2, beta = 7: the accumulators can only live in global memory; widths [2, 1], one row, rotations on both
    sides of N, against the schoolbook."""
    from tfhe_jl_amd import leveled
    N, k, l, beta = 8192, 1, 2, 7
    rng, sk, ck, eng, tgsw, tlwe = _setup(tfhe, N, k, l, beta, 7900, 2, 3)
    net = leveled.RotNet([2, 1], [[0, 1, 0, 0, 2 * N - 4096], [2, 1, 1, N + 5, 1], [1, 0, 1, 8191, 3]], N, entries=3, variables=2)
    sel = np.array([[1, 0]], np.int32)
    eng.tgsw_load(tgsw)
    got = eng.rot_net(tlwe, net, sel, out_form=0)
    assert eng.last_kernel_name() == f"rot_net_level_kernel(N={N},k={k},l={l},spec=global)"
    want, _ = ref_rows(Tree(N, k, l, beta, tgsw), net, tlwe[None], [0], sel)
    assert np.array_equal(got, want)
    ck.close()


# ---- 9. GPU: a packed table at full size -------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_packed_lookup_4096_entries_full_size(tfhe, keys80):
    """A random 4096-entry bit table under tfhe_parameters_80, packed into 4 samples, read through packed_lookup_net(12, 1024) (3 + 10
    external products) at 8 addresses, out_form 2: all 8 decrypt to the table entry and their gate_not to the opposite."""
    from tfhe_jl_amd import leveled
    K, d = keys80, 12
    p = K.params
    N, k, l = p.tlwe_polynomial_degree, p.tlwe_mask_size, p.bs_decomp_length
    rng = np.random.default_rng(8817)
    table = rng.integers(0, 2, 1 << d).astype(bool)
    data = leveled.pack_table_to_tlwe(table, N, k)
    net = leveled.packed_lookup_net(d, N)
    assert data.shape == (4, k + 1, N) and net.products == 13 and net.levels == 12
    addresses = np.array([0, 1, 1023, 1024, 2047, 2048, 4095, 2730])
    bits = (addresses[:, None] >> np.arange(d)) & 1
    tgsw = leveled.tgsw_encrypt_bits(rng, K.sk, bits.reshape(-1)).reshape(len(addresses), d, l, k + 1, k + 1, N)
    out = leveled.rot_net_lookup(K.ck, data, net, tgsw)
    want = table[addresses]
    assert len(out) == 8 and np.array_equal(tfhe.decrypt(K.sk, out), want)
    assert np.array_equal(tfhe.decrypt(K.sk, tfhe.gate_not(K.ck, out)), ~want)
    assert np.array_equal(tfhe.decrypt(K.sk, leveled.packed_lookup(K.ck, table, tgsw)), want)         # the same through packed_lookup


# ---- 10. GPU: the contract --------------------------------------------------------------------------------------------------------
def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class _Call:
    """A valid raw call of tfhe_rot_net_batch whose arguments can be replaced one at a time."""

    def __init__(self, eng, data, net, sel):
        self.eng, self.F = eng, int(net.widths[-1])
        self.base = dict(data=data, T=data.shape[0], E=data.shape[1], table_index=None, widths=net.widths, levels=net.levels, nodes=net.nodes,
                         sel=sel, V=sel.shape[1], B=sel.shape[0], out_form=0)

    def __call__(self, **over):
        a = dict(self.base, **over)
        out = np.zeros((self.base["B"], self.F) + self.base["data"].shape[2:], np.int32)
        rc = self.eng._lib.tfhe_rot_net_batch(self.eng._h, _ptr(a["data"]), a["T"], a["E"], _ptr(a["table_index"]), _ptr(a["widths"]), a["levels"],
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
    rng = np.random.default_rng(98)
    sk, ck = tfhe.make_key_pair(rng, p)
    eng = ck.engine(0)
    tg = leveled.tgsw_encrypt_bits(rng, sk, [1, 0, 1])
    data = leveled.tlwe_encrypt(rng, sk, _words(rng, E, N))[None]
    net = leveled.RotNet([2, 1], [[0, 1, 0, 3, 2 * N - 1], [2, 1, 1, N, 0], [1, 0, 1, 1, N + 1]], N, entries=E, variables=V)
    sel = np.array([[0, 1], [2, 0]], np.int32)
    want, want_ext = ref_rows(Tree(N, k, l, beta, tg), net, data, [0, 0], sel)
    call = _Call(eng, data, net, sel)

    def still_right():
        rc, msg, out = call()
        assert rc == 0 and np.array_equal(out, want), msg

    def refused(code, word, **over):
        rc, msg, _ = call(**over)
        assert rc == code and word in msg and "rot_net_batch" in msg, (over.keys(), rc, msg)
        still_right()

    rc, msg, _ = call()
    assert rc == NO_KEY and "selector" in msg                          # no selector set yet
    eng.tgsw_load(tg)
    still_right()
    bad = net.nodes.copy(); bad[1, 3] = -1
    refused(INVALID, "node 1 of level 0: rot0 = -1", nodes=bad)
    bad = net.nodes.copy(); bad[2, 4] = 2 * N
    refused(INVALID, f"node 0 of level 1: rot1 = {2 * N} is outside [0, {2 * N})", nodes=bad)
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
        raw.rot_net(data, net, sel, out_form=2)
    assert e.value.code == NO_KEY
    assert np.array_equal(raw.rot_net(data, net, sel, out_form=1), want_ext)
    raw.load_keyswitch_key(ck.keyswitch_key)
    assert np.array_equal(raw.rot_net(data, net, sel), eng.rot_net(data, net, sel))
    assert np.array_equal(eng.rot_net(data, net, sel).reshape(2, -1), eng.keyswitch(want_ext.reshape(2, -1)))
    raw.close()
    # a network for another polynomial degree never reaches the library
    with pytest.raises(ValueError, match="mod 2"):
        eng.rot_net(data, leveled.RotNet([1], [[0, 1, 0, 0, 0]], 2 * N), sel)
    # a multi-device context
    multi = ck.engine([0, 0])
    with pytest.raises(tfhe.EngineError) as e:
        multi.rot_net(data, net, sel)
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
def test_gpu_multikey_context_refuses_rot_net(tfhe):
    from test_independent import _mk_setup
    from tfhe_jl_amd import leveled
    p, sks, ck, xs, ys, want = _mk_setup(tfhe, 2, 4, 7, 3, 403)
    eng = ck.engine(0)
    net = leveled.RotNet([1], [[0, 1, 0, 1, 2]], 1024)
    with pytest.raises(tfhe.EngineError) as e:
        eng.rot_net(np.zeros((2, 2, 1024), np.int32), net, np.zeros((1, 1), np.int32))
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
    rng = np.random.default_rng(14)
    sk, ck = tfhe.make_key_pair(rng, p)
    eng = ck.engine(0)
    eng.tgsw_load(leveled.tgsw_encrypt_bits(rng, sk, [1]))
    table = leveled.pack_table_to_tlwe([False, True], N, k)
    small = leveled.packed_lookup_net(1, N)                           # selector bit 1: X^-1 brings entry 1 to coefficient 0
    assert list(tfhe.decrypt(sk, eng.rot_net(table, small, np.zeros((1, 1), np.int32))[:, 0])) == [True]
    B = 2**19 - 1
    nodes = np.zeros((4096 * 1024, 5), np.int32)
    nodes[:, 4] = 1
    huge = leveled.RotNet([4096] * 1024, nodes, N, entries=1, variables=1)
    sel = np.zeros((B, 1), np.int32)
    before = _mem_free()
    rc = eng._lib.tfhe_rot_net_batch(eng._h, _ptr(table), 1, 1, None, _ptr(huge.widths), huge.levels, _ptr(huge.nodes), _ptr(sel), 1,
                                     _ptr(np.zeros(1, np.int32)), B, 0)
    assert rc == NOMEM and "MB" in eng._lib.tfhe_last_error(eng._h).decode()
    assert _mem_free() == before
    assert list(tfhe.decrypt(sk, eng.rot_net(table, small, np.zeros((1, 1), np.int32))[:, 0])) == [True]
    ck.close()
