"""CMUX networks with monomial edges under a multi-key cloud key (tfhe_mk_rot_net_batch; Engine.mk_rot_net,
tfhe_jl_amd.leveled.mk_rot_net_lookup, mk_packed_lookup, packed_words_net, pack_words_to_tlwe) against an integer schoolbook network.

The reference of every word comparison is tests/test_rot_net.py's `rot_net_ref` over tests/test_mk_leveled.py's `MKTree`: `MKTree.cmux`
(exact int64, np.convolve, no transform, no rounding) per node on sources rotated by `rot` (X^r on every polynomial, coefficient by
coefficient), a rotated copy copying the rotated words, then `MKTree.extract` and `MKTree.keyswitch` — never the engine.  There are no
tolerances.

Noise (why "every address decrypts" is a condition, not a measurement): a rotation by a public monomial permutes and negates
coefficients and adds nothing, so a packed lookup carries the noise of its products alone: 8 multi-key external products at
(P, N, l, beta) = (2, 64, 3, 7) and depth 8, 13 at mktfhe_parameters_2party and depth 12 (1.8e-3 of the torus each,
tests/test_mk_leveled.py) against a window of 1/8.  The schoolbook alone is run on the CPU for every decrypting case below, the
full-size one at exactly the addresses of the GPU test.
"""
import functools
import os

import numpy as np
import pytest

from test_cmux_net import _mem_free, _ptr, random_net
from test_mk_leveled import MKTree, Setup, _gate_table, _words
from test_rot_net import random_rot_net, rot_net_ref as mk_rot_net_ref      # (duck-typed on ref.cmux: the one reference of tests/leveled_ref.py too)

INVALID, NO_KEY, STATE, NOMEM = 1, 3, 5, 6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tfhe_mk_rot_net_batch"


def ref_rows(ref, net, data, rows, sel, with_ks=False):
    """(samples [B][F][P+1][N], extracted [B][F][P N+1], keyswitched [B][F][P n+1] or None) of the schoolbook network, as int32."""
    want = np.stack([mk_rot_net_ref(ref, net, data[rows[g]], sel[g]) for g in range(len(sel))])
    ext = np.stack([[ref.extract(w) for w in row] for row in want])
    ks = np.stack([[ref.keyswitch(e) for e in row] for row in ext]).astype(np.int32) if with_ks else None
    return want.astype(np.int32), ext.astype(np.int32), ks


def _zero_rot(leveled, plain, N):
    """The CmuxNet `plain` as a RotNet with every rotation 0."""
    nodes = np.concatenate([plain.nodes, np.zeros((len(plain.nodes), 2), np.int32)], axis=1)
    return leveled.RotNet(plain.widths, nodes, N, entries=plain.entries, variables=plain.variables)


# ---- 1. CPU: the symbol -------------------------------------------------------------------------------------------------------------
def test_new_symbol_is_declared_bound_and_exported(tfhe):
    header = open(os.path.join(ROOT, "include", "tfhe_mi355x.h")).read()
    lib = tfhe._lib.load()
    assert NAME in tfhe._lib.ABI_SYMBOLS and f"int32_t {NAME}(tfhe_ctx *ctx" in header and hasattr(lib, NAME)
    assert len(lib.tfhe_mk_rot_net_batch.argtypes) == 13
    assert lib.tfhe_mk_rot_net_batch.argtypes == lib.tfhe_mk_cmux_net_batch.argtypes
    assert lib.tfhe_abi_version() == 7
    assert callable(tfhe.Engine.mk_rot_net) and callable(tfhe.leveled.mk_rot_net_lookup) and callable(tfhe.leveled.mk_packed_lookup)
    for fn in ("mk_rot_net_lookup", "mk_packed_lookup", "packed_words_net", "pack_words_to_tlwe"):
        assert fn in tfhe.__all__ and getattr(tfhe, fn) is getattr(tfhe.leveled, fn)


# ---- 2. CPU: the word builder in clear text ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,w,N,r", [(5, 4, 16, 2), (3, 2, 8, 2)])
def test_packed_words_net_clear_returns_every_bit_at_coefficient_0(tfhe, d, w, N, r):
    from tfhe_jl_amd import leveled
    net = leveled.packed_words_net(d, w, N)
    E = 1 << (d - r)
    assert net.entries == E and net.variables == d and net.levels == d + 1 and net.products == E - 1 + r
    assert list(net.widths) == [1 << (d - r - 1 - t) for t in range(d - r)] + [1] * r + [w]
    assert net.level(d - r).tolist() == [[0, 0, 0, 0, 2 * N - w]] and net.level(d - 1).tolist() == [[0, 0, r - 1, 0, 2 * N - (w << (r - 1))]]
    assert net.level(d)[:, 3:].tolist() == [[(2 * N - t) % (2 * N)] * 2 for t in range(w)] and not net.level(d)[:, :2].any()
    values = [int(v) for v in np.random.default_rng(d).integers(0, 1 << w, 1 << d)]
    values[0], values[-1] = (1 << w) - 1, 1 << (w - 1)
    tl = leveled.pack_words_to_tlwe(values, w, N, k=2, encode=lambda b: 5 + b)
    assert tl.shape == (E, 3, N) and tl.dtype == np.int32 and not tl[:, :2].any()
    for i, v in enumerate(values):                                       # bit t of entry i on coefficient w (i mod 2^r) + t of sample i >> r
        assert tl[i >> r, 2, w * (i % (1 << r)):w * (i % (1 << r)) + w].tolist() == [5 + ((v >> t) & 1) for t in range(w)]
    assert not tl[:, 2, w << r:].any()
    for address in range(1 << d):
        out = net.evaluate_clear(tl[:, 2].astype(np.int64), [(address >> v) & 1 for v in range(d)])
        assert len(out) == w and [int(o[0]) for o in out] == [5 + ((values[address] >> t) & 1) for t in range(w)], address


def test_packed_words_net_with_one_bit_words_is_packed_lookup_net(tfhe):
    from tfhe_jl_amd import leveled
    for d, N in ((5, 8), (3, 8), (12, 1024), (2, 64)):
        a, b = leveled.packed_words_net(d, 1, N), leveled.packed_lookup_net(d, N)
        assert np.array_equal(a.nodes, b.nodes) and np.array_equal(a.widths, b.widths) and (a.entries, a.variables) == (b.entries, b.variables)
    bits = [True, False, True, True]
    assert np.array_equal(leveled.pack_words_to_tlwe(bits, 1, 8, k=2), leveled.pack_table_to_tlwe(bits, 8, k=2))
    whole = leveled.packed_words_net(3, 8, 8)                            # w = N: no rotation stage, a tree and the copies
    assert list(whole.widths) == [4, 2, 1, 8] and whole.entries == 8 and whole.products == 7
    for bad in (0, 3, 6, 16, -2):
        with pytest.raises(ValueError, match="word_bits"):
            leveled.packed_words_net(3, bad, 8)
        with pytest.raises(ValueError, match="word_bits"):
            leveled.pack_words_to_tlwe([1, 2], bad, 8)
    with pytest.raises(ValueError, match="N = 12"):
        leveled.packed_words_net(3, 2, 12)
    for depth, w, n in ((0, 2, 8), (25, 2, 1 << 13), (15, 2, 8)):        # 2^13 table samples at (15, 2, 8)
        with pytest.raises(ValueError, match="depth"):
            leveled.packed_words_net(depth, w, n)
    with pytest.raises(ValueError, match="2\\^depth entries"):
        leveled.pack_words_to_tlwe([1, 2, 3], 2, 8)


# ---- 3. CPU: the schoolbook alone decrypts a packed lookup at every address ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _packed_case(tfhe, orc):
    """(P, N, l, beta) = (2, 64, 3, 7), packed_lookup_net(8, 64): address bit v is owned by party v mod 2, selector 2 v + bit encrypts
    `bit`; 256 random bits packed into 4 samples, once trivial and once encrypted; the schoolbook's words for all 256 addresses in both
    tables, computed once for the CPU and the GPU test."""
    from tfhe_jl_amd import leveled
    P, N, l, beta, d = 2, 64, 3, 7, 8
    owners = [v % 2 for v in range(d) for _ in (0, 1)]
    s = Setup(tfhe, P, N, l, beta, 4242, owners, bits=[0, 1] * d)
    bits = np.random.default_rng(5).integers(0, 2, 1 << d).astype(bool)
    trivial = leveled.pack_table_to_tlwe(bits, N, k=P)
    data = np.stack([trivial, s.encrypt(trivial[:, P, :])])              # [2][4][P+1][N]
    net = leveled.packed_lookup_net(d, N)
    sel = np.array([[2 * v + ((a >> v) & 1) for v in range(d)] for a in range(1 << d)], np.int32)
    ref = s.tree(orc, with_ks=True)
    want = [ref_rows(ref, net, data, [t] * len(sel), sel, with_ks=True) for t in (0, 1)]
    return s, bits, data, net, sel, want


def test_schoolbook_packed_lookup_decrypts_every_address(tfhe, orc):
    """2 tree levels and 6 rotation levels: the phase at coefficient 0 has the sign of the entry and lies within 2^28 (1/16 of the
    torus, test_mk_leveled's bound) of +-2^29, for all 256 addresses of the trivial and of the encrypted table."""
    from tfhe_jl_amd import leveled
    s, bits, data, net, sel, want = _packed_case(tfhe, orc)
    assert data.shape == (2, 4, 3, 64) and list(net.widths) == [2, 1] + [1] * 6 and net.products == 9
    target = np.where(bits, 2**29, -2**29)
    for t in (0, 1):
        phase = leveled.mk_tlwe_phase(s.tlwe_keys, want[t][0][:, 0])[:, 0].astype(np.int64)
        err = np.abs(phase - target).max()
        print(f"table {t}: worst phase error at coefficient 0: 2^{np.log2(max(err, 1)):.1f}")
        assert np.array_equal(phase > 0, bits), t
        assert err < 2**28, (t, err)


# ---- 4. CPU: the schoolbook alone decrypts f(popcount) of bits of three parties ------------------------------------------------------
def _popcount_case(tfhe, trial):
    from tfhe_jl_amd import leveled
    P, N, l, beta, steps = 3, 64, 3, 7, 15
    rng = np.random.default_rng(9)
    inputs = [[0] * steps, [1] * steps] + [[int(b) for b in rng.integers(0, 2, steps)] for _ in range(10)]
    net = leveled.wfa_net([0], [0], [0], [2 * N - 1], 0, steps, N)
    mu = np.array([[leveled.encode_gate_bit(c >= 8) for c in range(N)]], np.int32)
    s = Setup(tfhe, P, N, l, beta, 900 + trial, owners=[v % P for v in range(steps)], bits=inputs[trial])
    return s, net, leveled.mk_tlwe_trivial(mu, P), inputs[trial]


def test_schoolbook_popcount_threshold_over_three_parties(tfhe, orc):
    """One state, 15 letters, weights 0 and 2N - 1: X^(-popcount) tv with tv[c] = (c >= 8), gate-encoded, on a trivial sample; bit v is
    owned by party v mod 3.  All 12 inputs give "at least 8 of the 15 bits are set" with the phase within 2^28 of +-2^29."""
    from tfhe_jl_amd import leveled
    worst = 0
    for trial in range(12):
        s, net, table, bits = _popcount_case(tfhe, trial)
        assert net.products == 15 and len(net.evaluate_clear([table[0, 3].astype(np.int64)], bits)) == 1
        got = mk_rot_net_ref(s.tree(orc), net, table, list(range(15)))
        phase = int(leveled.mk_tlwe_phase(s.tlwe_keys, got[0].astype(np.int32))[0, 0])
        truth = sum(bits) >= 8
        err = abs(phase - (2**29 if truth else -2**29))
        worst = max(worst, err)
        assert (phase > 0) == truth and err < 2**28, (trial, bits, phase)
        s.ck.close()
    print(f"worst phase error at coefficient 0: 2^{np.log2(max(worst, 1)):.1f}")


# ---- 13 (CPU part). the schoolbook alone at the full-size shape, for exactly the addresses of the GPU test --------------------------
def _full_case():
    rng = np.random.default_rng(8803)
    table = rng.integers(0, 2, 4096).astype(bool)
    addresses = np.array([0, 4095, 1023, 1024] + [int(a) for a in rng.integers(0, 4096, 4)])
    return table, addresses


def test_schoolbook_packed_lookup_full_size_addresses(tfhe, orc):
    """N = 1024, l = 4, beta = 7, bs noise 3.29e-10 (mktfhe_parameters_2party's ring), packed_lookup_net(12, 1024): 3 tree products and
    10 rotation products; bit v owned by party v mod 2.  All 8 addresses of the GPU test decrypt inside the +-1/8 window."""
    from tfhe_jl_amd import leveled
    P, N, l, beta, d = 2, 1024, 4, 7, 12
    table, addresses = _full_case()
    s = Setup(tfhe, P, N, l, beta, 8804, owners=[v % 2 for v in range(d) for _ in (0, 1)], bits=[0, 1] * d)
    data = leveled.pack_table_to_tlwe(table, N, k=P)
    net = leveled.packed_lookup_net(d, N)
    assert data.shape == (4, P + 1, N) and list(net.widths) == [2] + [1] * 11 and net.products == 13
    ref = s.tree(orc)
    worst = 0
    for a in addresses:
        got = mk_rot_net_ref(ref, net, data, [2 * v + ((int(a) >> v) & 1) for v in range(d)])
        phase = int(leveled.mk_tlwe_phase(s.tlwe_keys, got[0].astype(np.int32))[0, 0])
        err = abs(phase - (2**29 if table[a] else -2**29))
        worst = max(worst, err)
        assert (phase > 0) == table[a] and err < 2**29, (a, phase)
    print(f"worst phase error: {worst / 2**32:.2e} of the torus")
    s.ck.close()


# ---- 5. GPU: a random rotated network word for word ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("P,N,l,beta", [(2, 64, 3, 7), (3, 32, 2, 8), (4, 64, 2, 10), (2, 1024, 4, 7)])
def test_gpu_mk_random_rot_network_equals_schoolbook(tfhe, orc, P, N, l, beta):
    from tfhe_jl_amd import leveled
    B, T, E, V = 3, 2, 5, 4
    owners = [0, 1, 2 % P, P - 1, 1, 0]                                  # every party owns a selector
    s = Setup(tfhe, P, N, l, beta, 6300 + P + N + l, owners)
    eng = s.ck.engine(0)
    data = s.encrypt(_words(s.rng, T * E, N)).reshape(T, E, P + 1, N)
    net = random_rot_net(leveled, s.rng, N, E, V)
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
        got0 = eng.mk_rot_net(data, net, sel, table_index=idx, out_form=0)
        assert got0.shape == (B, 2, P + 1, N) and np.array_equal(got0, want), ("out_form 0", idx)
        assert eng.last_kernel_name() == f"mk_rot_net_level_kernel(N={N},P={P},l={l})"
        assert eng.last_rotation_count() == 0 and eng.last_timing_ms(0) > 0
        got1 = eng.mk_rot_net(data, net, sel, table_index=idx, out_form=1)
        assert got1.shape == (B, 2, P * N + 1) and np.array_equal(got1, want_ext), ("out_form 1", idx)
        got2 = eng.mk_rot_net(data, net, sel, table_index=idx, out_form=2)
        assert eng.last_timing_ms(1) > 0 and got2.shape == (B, 2, P * s.n + 1)
        assert np.array_equal(got2, want_ks), ("out_form 2", idx)
    s.ck.close()


# ---- 6. GPU: rotated copies never pass through floating point -----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("P,N,l,beta", [(2, 64, 3, 7), (3, 32, 2, 8)])
def test_gpu_mk_rotated_copies_on_arbitrary_words(tfhe, orc, P, N, l, beta):
    """A network of rotated copies only, two levels deep, on arbitrary Int32 tables with all-(-2^31), all-(2^31 - 1) and all-zero
    samples: the exact words of the host's rotation (the negation of -2^31 is -2^31), as samples and extracted — with P = 3 the
    extraction of every party's mask."""
    from tfhe_jl_amd import leveled
    E = 5
    s = Setup(tfhe, P, N, l, beta, 7400 + P, owners=[0, 1])
    eng = s.ck.engine(0)
    data = _words(s.rng, 2, E, P + 1, N)
    data[0, 0], data[0, 1], data[0, 2] = -2**31, 2**31 - 1, 0
    data[1, 4, 0], data[1, 4, P, ::2] = -2**31, -2**31
    rots = [1, N, 2 * N - 1]
    level0 = [[e, e, 0, rots[e % 3], rots[e % 3]] for e in range(E)] + [[0, 0, 0, N, N]]
    level1 = [[i, i, 0, rots[(i + 1) % 3], rots[(i + 1) % 3]] for i in (5, 0, 1, 4)]
    net = leveled.RotNet([6, 4], level0 + level1, N, entries=E, variables=1)
    assert net.products == 0
    index = np.array([0, 1, 0], np.int32)
    sel = np.zeros((3, 1), np.int32)
    want, want_ext, _ = ref_rows(s.tree(orc), net, data, index, sel)
    assert np.array_equal(want[0, 0], np.full((P + 1, N), -2**31))                       # X^N X^N (-2^31 ...) in 32-bit words
    eng.mk_tgsw_load(s.tgsw, s.owners)
    assert np.array_equal(eng.mk_rot_net(data, net, sel, table_index=index, out_form=0), want)
    assert np.array_equal(eng.mk_rot_net(data, net, sel, table_index=index, out_form=1), want_ext)
    s.ck.close()


# ---- 7. GPU: with every rotation 0 the network is tfhe_mk_cmux_net_batch ------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("P,N,l,beta", [(2, 64, 3, 7), (3, 32, 2, 8)])
def test_gpu_mk_zero_rotations_equal_mk_cmux_net_and_tree(tfhe, orc, P, N, l, beta):
    """Word for word in every form, also where the set is not exact for arbitrary words ((3, 32, 2, 8)): the kernels make the same
    floating-point operations in the same order."""
    from tfhe_jl_amd import leveled
    B, T, E, V, widths = 3, 2, 8, 4, [4, 3, 2]
    owners = list(range(P)) + [P - 1, 0, 1]
    s = Setup(tfhe, P, N, l, beta, 7500 + P + N, owners)
    eng = s.ck.engine(0)
    full = s.encrypt(_words(s.rng, T * E, N)).reshape(T, E, P + 1, N)
    arbitrary = _words(s.rng, T, E, P + 1, N)
    arbitrary[0, 1], arbitrary[1, 2], arbitrary[1, 3] = 2**31 - 1, -2**31, 0
    plain = leveled.CmuxNet(widths, random_net(s.rng, 5, widths, V), entries=E, variables=V)
    tree = leveled.tree_net(3)
    sel = np.array([[0, 1, 2, 3], [5, 4, 0, 2], [3, 3, 1, 5]], np.int32) % len(owners)
    index = np.array([1, 0, 1], np.int32)
    eng.mk_tgsw_load(s.tgsw, s.owners)
    for data in (full, arbitrary):
        for form in (0, 1, 2):
            a = eng.mk_cmux_net(data, plain, sel, table_index=index, out_form=form)
            b = eng.mk_rot_net(data, _zero_rot(leveled, plain, N), sel, table_index=index, out_form=form)
            assert a.shape == b.shape and np.array_equal(a, b), ("net", form)
            t = eng.mk_cmux_tree(data, sel[:, :3], table_index=index, out_form=form)
            b = eng.mk_rot_net(data, _zero_rot(leveled, tree, N), sel[:, :3], table_index=index, out_form=form)
            assert b.shape == (B, 1) + t.shape[1:] and np.array_equal(b[:, 0], t), ("tree", form)
    want, _, _ = ref_rows(s.tree(orc), _zero_rot(leveled, plain, N), full, index[:1], sel[:1])       # ... and they are the schoolbook's words
    assert np.array_equal(eng.mk_rot_net(full, _zero_rot(leveled, plain, N), sel[:1], table_index=index[:1], out_form=0), want)
    s.ck.close()


# ---- 8. GPU: spectrum accumulators in global memory ---------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_mk_rot_accumulators_in_global_memory_small(tfhe, orc):
    from tfhe_jl_amd import leveled
    P, N, l, beta, E, V = 2, 64, 3, 7, 5, 4
    s = Setup(tfhe, P, N, l, beta, 7800, owners=[1, 0, 1, 0, 0, 1])
    eng = s.ck.engine(0)
    data = s.encrypt(_words(s.rng, E, N))
    net = random_rot_net(leveled, s.rng, N, E, V)
    sel = np.array([[0, 1, 2, 3], [5, 4, 0, 2]], np.int32)
    eng.mk_tgsw_load(s.tgsw, s.owners)
    lds = [eng.mk_rot_net(data, net, sel, out_form=f) for f in (0, 1, 2)]
    assert eng.last_kernel_name() == f"mk_rot_net_level_kernel(N={N},P={P},l={l})"
    eng.set_option("anyn_spec", 1)
    glob = [eng.mk_rot_net(data, net, sel, out_form=f) for f in (0, 1, 2)]
    assert eng.last_kernel_name() == f"mk_rot_net_level_kernel(N={N},P={P},l={l},spec=global)"
    for a, b in zip(lds, glob):
        assert np.array_equal(a, b)
    want, want_ext, want_ks = ref_rows(s.tree(orc, with_ks=True), net, data[None], [0, 0], sel, with_ks=True)
    assert np.array_equal(glob[0], want) and np.array_equal(glob[1], want_ext) and np.array_equal(glob[2], want_ks)
    s.ck.close()


@pytest.mark.gpu
def test_gpu_mk_rot_accumulators_in_global_memory_n4096(tfhe, orc):
    """N = 4096 at P = 2: the three accumulators can only live in global memory (tests/test_mk_leveled.py); one row, two products and a
    rotated copy, an odd rotation and N + 1, against the schoolbook."""
    from tfhe_jl_amd import leveled
    P, N, l, beta = 2, 4096, 2, 6
    s = Setup(tfhe, P, N, l, beta, 7900, owners=[1, 0], n=2)
    eng = s.ck.engine(0)
    data = s.encrypt(_words(s.rng, 3, N))
    net = leveled.RotNet([2, 1], [[0, 1, 0, 0, 2 * N - 5], [2, 2, 1, N + 1, N + 1], [1, 0, 1, N + 1, 3]], N, entries=3, variables=2)
    assert net.products == 2
    sel = np.array([[1, 0]], np.int32)
    eng.mk_tgsw_load(s.tgsw, s.owners)
    got = eng.mk_rot_net(data, net, sel, out_form=0)
    assert eng.last_kernel_name() == f"mk_rot_net_level_kernel(N={N},P={P},l={l},spec=global)"
    want, _, _ = ref_rows(s.tree(orc), net, data[None], [0], sel)
    assert np.array_equal(got, want)
    s.ck.close()


# ---- 9. GPU: a packed lookup at every address ---------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_mk_packed_lookup_every_address(tfhe, orc):
    """mk_packed_lookup at B = 256, one row per address, the selectors expanded on the device from the parties' uni-encryptions: word
    for word against the schoolbook of the CPU test above in forms 0 and 1, against MKTree.keyswitch in form 2."""
    from tfhe_jl_amd import leveled
    s, bits, data, net, sel, want = _packed_case(tfhe, orc)
    P, N = s.P, s.N
    uni = [a[sel] for a in s.uni]                                        # [256][8][l][N]: the uni-encryption behind every (row, bit)
    party_of = s.owners[sel[0]]                                          # bit v: party v mod 2, whatever its value
    assert uni[0].shape == (256, 8, s.l, N) and party_of.tolist() == [0, 1] * 4
    for t, table in ((0, bits), (1, data[1])):                           # plain values packed by the call; the encrypted samples as they are
        w, w_ext, w_ks = want[t]
        got0 = leveled.mk_packed_lookup(s.ck, table, uni, party_of, out_form=0)
        assert got0.shape == (256, P + 1, N) and np.array_equal(got0, w[:, 0]), t
        assert s.ck.engine(0).last_kernel_name() == f"mk_rot_net_level_kernel(N={N},P={P},l={s.l})"
        assert np.array_equal(leveled.mk_packed_lookup(s.ck, table, uni, party_of, out_form=1), w_ext[:, 0]), t
        got2 = leveled.mk_packed_lookup(s.ck, table, uni, party_of)
        assert got2.shape == (256, P * s.n + 1) and np.array_equal(got2, w_ks[:, 0]), t
        assert np.array_equal(leveled.mk_packed_lookup(s.ck, table, [a[:3] for a in uni], party_of, out_form=1, expand="host"), w_ext[:3, 0]), t
        phase = leveled.mk_tlwe_phase(s.tlwe_keys, got0)[:, 0]
        assert np.array_equal(phase > 0, bits), t
    with pytest.raises(ValueError, match="4 samples"):
        leveled.mk_packed_lookup(s.ck, data[1][:2], uni, party_of)


# ---- 10. GPU: the word builder on both engines --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_packed_words_net_on_both_engines(tfhe, orc):
    """packed_words_net(5, 4, 64): E = 2 samples, one tree level, four rotation levels and the level of four rotated copies; F = 4
    outputs per row, word for word against the single-key and the multi-key schoolbook."""
    from tfhe_jl_amd import leveled
    from test_leveled import Tree, _setup
    from test_rot_net import ref_rows as sk_ref_rows
    d, w, N = 5, 4, 64
    net = leveled.packed_words_net(d, w, N)
    assert list(net.widths) == [1, 1, 1, 1, 1, 4] and net.entries == 2 and net.products == 5
    values = [int(v) for v in np.random.default_rng(54).integers(0, 16, 32)]
    sel = np.array([[0, 1, 2, 3, 4], [5, 4, 0, 2, 1], [3, 3, 1, 5, 0]], np.int32)
    # single-key, (N, k, l, beta) = (64, 1, 3, 8)
    rng, sk, ck, eng, tgsw, _ = _setup(tfhe, N, 1, 3, 8, 5400, 6, 3)
    data = leveled.pack_words_to_tlwe(values, w, N, k=1)
    want, want_ext = sk_ref_rows(Tree(N, 1, 3, 8, tgsw), net, data[None], [0] * 3, sel)
    eng.tgsw_load(tgsw)
    got = eng.rot_net(data, net, sel, out_form=0)
    assert got.shape == (3, 4, 2, N) and np.array_equal(got, want)
    assert np.array_equal(eng.rot_net(data, net, sel, out_form=1), want_ext)
    ck.close()
    # multi-key, (P, N, l, beta) = (2, 64, 3, 7)
    P = 2
    s = Setup(tfhe, P, N, 3, 7, 5401, owners=[0, 1, 0, 1, 1, 0])
    eng = s.ck.engine(0)
    data = leveled.pack_words_to_tlwe(values, w, N, k=P)
    want, want_ext, want_ks = ref_rows(s.tree(orc, with_ks=True), net, data[None], [0] * 3, sel, with_ks=True)
    eng.mk_tgsw_load(s.tgsw, s.owners)
    got = eng.mk_rot_net(data, net, sel, out_form=0)
    assert got.shape == (3, 4, P + 1, N) and np.array_equal(got, want)
    assert np.array_equal(eng.mk_rot_net(data, net, sel, out_form=1), want_ext)
    assert np.array_equal(eng.mk_rot_net(data, net, sel, out_form=2), want_ks)
    s.ck.close()


# ---- 11. GPU: workspaces sized by every level, regrown correctly, shared with the tree ----------------------------------------------
@pytest.mark.gpu
def test_gpu_mk_rot_workspace_parity_and_regrowth(tfhe, orc):
    """Widths [2, 6, 3, 7, 1] as the first call of a fresh context (the odd levels are wider than level 0 and than every even level),
    then a one-node network, then the first again, all with non-zero rotations, then a CMUX tree on the same context and buffers."""
    from tfhe_jl_amd import leveled
    P, N, l, beta, B, E, V = 2, 64, 3, 7, 2, 4, 5
    s = Setup(tfhe, P, N, l, beta, 6500, owners=[0, 1, 1, 0, 1])
    eng = s.ck.engine(0)
    data = s.encrypt(_words(s.rng, E, N)).reshape(1, E, P + 1, N)
    widths = [2, 6, 3, 7, 1]
    nodes = []
    for v, w in enumerate(widths):
        below = E if v == 0 else widths[v - 1]
        nodes += [[i % below, (i + 1 + v) % below if below > 1 else 0, (i + v) % V, 1 + (37 * i + 11 * v) % (2 * N - 1), 1 + (53 * i + 29 * v) % (2 * N - 1)]
                  for i in range(w)]
    big = leveled.RotNet(widths, nodes, N, entries=E, variables=V)
    one = leveled.RotNet([1], [[2, 0, 4, N + 3, 7]], N, entries=E, variables=V)
    sel = np.array([[0, 1, 2, 3, 4], [4, 2, 0, 1, 3]], np.int32)
    ref = s.tree(orc)
    eng.mk_tgsw_load(s.tgsw, s.owners)
    for net in (big, one, big):
        want, want_ext, _ = ref_rows(ref, net, data, [0] * B, sel)
        assert np.array_equal(eng.mk_rot_net(data, net, sel, out_form=0), want), list(net.widths)
        assert np.array_equal(eng.mk_rot_net(data, net, sel, out_form=1), want_ext), list(net.widths)
    tree = np.stack([ref.tree(data[0], sel[g, :2]) for g in range(B)])
    assert np.array_equal(eng.mk_cmux_tree(data, sel[:, :2], out_form=0), tree.astype(np.int32))
    want, _, _ = ref_rows(ref, big, data, [0] * B, sel)
    assert np.array_equal(eng.mk_rot_net(data, big, sel, out_form=0), want)
    s.ck.close()


# ---- 12. GPU: the contract ----------------------------------------------------------------------------------------------------------
class _Call:
    """A valid raw call of tfhe_mk_rot_net_batch whose arguments can be replaced one at a time."""

    def __init__(self, eng, data, net, sel):
        self.eng, self.F = eng, int(net.widths[-1])
        self.base = dict(data=data, T=data.shape[0], E=data.shape[1], table_index=None, widths=net.widths, levels=net.levels, nodes=net.nodes,
                         sel=sel, V=sel.shape[1], B=sel.shape[0], out_form=0)

    def __call__(self, eng=None, **over):
        eng = eng or self.eng
        a = dict(self.base, **over)
        out = np.zeros((self.base["B"], self.F) + self.base["data"].shape[2:], np.int32)
        rc = eng._lib.tfhe_mk_rot_net_batch(eng._h, _ptr(a["data"]), a["T"], a["E"], _ptr(a["table_index"]), _ptr(a["widths"]), a["levels"],
                                            _ptr(a["nodes"]), _ptr(a["sel"]), a["V"], _ptr(a.get("out", out)), a["B"], a["out_form"])
        return rc, eng._lib.tfhe_last_error(eng._h).decode(), out


@pytest.mark.gpu
def test_gpu_mk_rot_contract_refusals_leave_the_context_usable(tfhe, orc):
    from tfhe_jl_amd import leveled
    P, N, l, beta, E, V, S = 2, 64, 3, 7, 3, 2, 3
    s = Setup(tfhe, P, N, l, beta, 9700, owners=[0, 1, 0])
    eng = s.ck.engine(0)
    data = s.encrypt(_words(s.rng, E, N))[None]
    net = leveled.RotNet([2, 1], [[0, 1, 0, 3, 2 * N - 1], [2, 2, 1, N, N], [1, 0, 1, 1, N + 1]], N, entries=E, variables=V)
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
        assert rc == code and word in msg and "mk_rot_net_batch" in msg, (over.keys(), rc, msg)
        still_right()

    rc, msg, _ = call()
    assert rc == NO_KEY and "selector" in msg                          # no selector set yet
    nand_works(eng)
    eng.mk_tgsw_load(s.tgsw, s.owners)
    still_right()
    # 1. NULL arguments, a negative B
    for name in ("data", "widths", "nodes", "sel", "out"):
        refused(INVALID, "NULL", **{name: None})
    refused(INVALID, "negative", B=-1)
    # 3. the netlist, with the messages of the record check
    bad = net.nodes.copy(); bad[1, 3] = -1
    refused(INVALID, "node 1 of level 0: rot0 = -1", nodes=bad)
    bad = net.nodes.copy(); bad[2, 4] = 2 * N
    refused(INVALID, f"node 0 of level 1: rot1 = {2 * N} is outside [0, {2 * N})", nodes=bad)
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
    for form in (3, -1):
        refused(INVALID, "out_form", out_form=form)
    refused(INVALID, "exceed one launch", B=2**30)                     # B * widths[0] = 2^31 (refused before sel is read)
    # 5. the rows
    for sidx in (S, -1):
        bad = sel.copy(); bad[1, 0] = sidx
        refused(INVALID, "sel[1][0]", sel=bad)
    for t in (1, -1):
        refused(INVALID, "table_index[1]", table_index=np.array([0, t], np.int32))
    # 6. B = 0
    rc, msg, _ = call(B=0, data=None, sel=None)
    assert rc == 0
    # 2. the state
    eng.set_option("measure_margin", 1)
    rc, msg, _ = call()
    assert rc == STATE and "measure_margin" in msg
    eng.set_option("measure_margin", 0)
    still_right()
    assert np.array_equal(eng.mk_rot_net(data, net, sel, out_form=1), want_ext) and np.array_equal(eng.mk_rot_net(data, net, sel), want_ks)
    # a network for another polynomial degree never reaches the library
    with pytest.raises(ValueError, match="mod 2"):
        eng.mk_rot_net(data, leveled.RotNet([1], [[0, 1, 0, 0, 0]], 2 * N), sel)
    # no multi-key bootstrapping key, then no selector set, then (4.) out_form 2 without the multi-key keyswitch key; forms 0 and 1 do
    # not need it, and a bad netlist is named before the missing keyswitch key
    raw = tfhe.Engine(s.p)
    rc, msg, _ = call(raw)
    assert rc == NO_KEY and "bootstrapping key" in msg
    raw.mk_load_bootstrap_key(s.ck.bootstrap_key, P)
    rc, msg, _ = call(raw)
    assert rc == NO_KEY and "selector" in msg
    raw.mk_tgsw_load(s.tgsw, s.owners)
    rc, msg, _ = call(raw, out_form=2)
    assert rc == NO_KEY and "keyswitch" in msg
    bad = net.nodes.copy(); bad[0, 3] = 2 * N
    rc, msg, _ = call(raw, out_form=2, nodes=bad)
    assert rc == INVALID and "rot0" in msg
    assert np.array_equal(raw.mk_rot_net(data, net, sel, out_form=1), want_ext)
    raw.mk_load_keyswitch_key(s.ck.keyswitch_key, P)
    assert np.array_equal(raw.mk_rot_net(data, net, sel), want_ks)
    raw.close()
    # 4., the other half: out_form 2 with a keyswitch key made for another party count (bootstrapping key for 3 parties, keyswitch key
    # for 2, as tests/test_abi_nomem.py builds them): TFHE_ERR_STATE, after the netlist; forms 0 and 1 do not read that key
    s3 = Setup(tfhe, 3, 32, 2, 8, 9701, owners=[0, 1, 2])
    ck2 = tfhe.MKCloudKey(s3.parts[:2])
    N3 = s3.N
    data3 = s3.encrypt(_words(s3.rng, E, N3))[None]
    net3 = leveled.RotNet([2, 1], [[0, 1, 0, 3, 2 * N3 - 1], [2, 2, 1, N3, N3], [1, 0, 1, 1, N3 + 1]], N3, entries=E, variables=V)
    want3, want3_ext, want3_ks = ref_rows(s3.tree(orc, with_ks=True), net3, data3, [0, 0], sel, with_ks=True)
    raw3 = tfhe.Engine(s3.p)
    raw3.mk_load_bootstrap_key(s3.ck.bootstrap_key, 3)
    raw3.mk_tgsw_load(s3.tgsw, s3.owners)
    raw3.mk_load_keyswitch_key(ck2.keyswitch_key, 2)
    call3 = _Call(raw3, data3, net3, sel)
    rc, msg, _ = call3(out_form=2)
    assert rc == STATE and "parties" in msg and "mk_rot_net_batch" in msg, (rc, msg)
    bad = net3.nodes.copy(); bad[0, 3] = 2 * N3
    rc, msg, _ = call3(out_form=2, nodes=bad)
    assert rc == INVALID and "rot0" in msg, (rc, msg)
    rc, msg, out = call3()
    assert rc == 0 and np.array_equal(out, want3), msg
    assert np.array_equal(raw3.mk_rot_net(data3, net3, sel, out_form=1), want3_ext)
    raw3.mk_load_keyswitch_key(s3.ck.keyswitch_key, 3)
    assert np.array_equal(raw3.mk_rot_net(data3, net3, sel), want3_ks)
    raw3.close()
    ck2.close()
    s3.ck.close()
    # a single-key context: the new call is refused, its gates go on
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
def test_gpu_mk_rot_oversized_network_is_refused_before_allocating(tfhe):
    """1024 levels of 4096 nodes at B = 2^19 - 1 rows: one workspace alone is 1.6 TB.  TFHE_ERR_NOMEM, computed and refused before any
    allocation (hipMemGetInfo reads unchanged), and the context goes on working."""
    from tfhe_jl_amd import leveled
    P, N, l, beta = 2, 64, 3, 7
    s = Setup(tfhe, P, N, l, beta, 9800, owners=[1], bits=[1])
    eng = s.ck.engine(0)
    eng.mk_tgsw_load(s.tgsw, s.owners)
    table = leveled.pack_table_to_tlwe([False, True], N, k=P)
    small = leveled.packed_lookup_net(1, N)                           # selector bit 1: X^-1 brings entry 1 to coefficient 0
    assert list(tfhe.mk_decrypt(s.sks, eng.mk_rot_net(table, small, np.zeros((1, 1), np.int32))[:, 0])) == [True]
    B = 2**19 - 1
    nodes = np.zeros((4096 * 1024, 5), np.int32)
    nodes[:, 4] = 1
    huge = leveled.RotNet([4096] * 1024, nodes, N, entries=1, variables=1)
    sel = np.zeros((B, 1), np.int32)
    before = _mem_free()
    rc = eng._lib.tfhe_mk_rot_net_batch(eng._h, _ptr(table), 1, 1, None, _ptr(huge.widths), huge.levels, _ptr(huge.nodes), _ptr(sel), 1,
                                        _ptr(np.zeros(1, np.int32)), B, 0)
    assert rc == NOMEM and "MB" in eng._lib.tfhe_last_error(eng._h).decode()
    assert _mem_free() == before
    assert list(tfhe.mk_decrypt(s.sks, eng.mk_rot_net(table, small, np.zeros((1, 1), np.int32))[:, 0])) == [True]
    s.ck.close()


# ---- 13. GPU: a packed table at full size -------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_mk_packed_lookup_4096_entries_full_size(tfhe, orc):
    """mktfhe_parameters_2party, a random 4096-entry bit table packed into 4 samples, packed_lookup_net(12, 1024) (3 + 10 multi-key
    external products) at 8 addresses, bit v owned by party v mod 2, the 96 selectors expanded on the device, out_form 2: mk_decrypt
    returns table[address] for all 8, the answers NANDed with fresh encryptions decrypt too; row 0 at out_form 1 with the host expansion
    equals the extraction of the schoolbook network word for word."""
    from tfhe_jl_amd import leveled
    p = tfhe.mktfhe_parameters_2party
    N, l, beta, P, d = p.tlwe_polynomial_degree, p.bs_decomp_length, p.bs_log2_base, 2, 12
    assert (N, l, beta) == (1024, 4, 7)
    table, addresses = _full_case()
    rng = np.random.default_rng(8805)
    sks = [tfhe.SecretKey(rng, p) for _ in range(P)]
    shared = tfhe.SharedKey(rng, p)
    parts = [tfhe.CloudKeyPart(rng, sk, shared, keep_tlwe_key=True) for sk in sks]
    ck = tfhe.MKCloudKey(parts, expand="device")
    owners = np.array([v % 2 for v in range(d)], np.int32)
    abits = (addresses[:, None] >> np.arange(d)[None, :]) & 1
    uni = [np.zeros((8, d, l, N), np.int32) for _ in range(6)]
    for i in range(P):
        cols = np.nonzero(owners == i)[0]
        arrs = leveled.mk_tgsw_uni_encrypt_bits(rng, parts[i].tlwe_key, shared, parts[i].public_b, abits[:, cols].reshape(-1))
        for dst, a in zip(uni, arrs):
            dst[:, cols] = a.reshape(8, cols.size, l, N)
    out = leveled.mk_packed_lookup(ck, table, uni, owners)
    assert out.shape == (8, P * p.lwe_size + 1)
    assert ck.engine(0).last_kernel_name() == f"mk_rot_net_level_kernel(N={N},P={P},l={l})"
    assert np.array_equal(tfhe.mk_decrypt(sks, out), table[addresses])
    y = rng.integers(0, 2, 8).astype(bool)
    nand = tfhe.mk_gate_nand(ck, out, tfhe.mk_encrypt(rng, sks, y))
    assert np.array_equal(tfhe.mk_decrypt(sks, nand), ~(table[addresses] & y))
    pub = np.stack([part.public_b for part in parts])
    tg = np.zeros((d, 2 * l * P + 2 * l, N), np.int32)
    for v in range(d):
        tg[v] = leveled.mk_tgsw_expand(p, pub, owners[v], *[a[0, v:v + 1] for a in uni])[0]
    ref = MKTree(orc, N, l, beta, P, tg, owners)
    net = leveled.packed_lookup_net(d, N)
    data = leveled.pack_table_to_tlwe(table, N, k=P)
    ext = leveled.mk_packed_lookup(ck, data, [a[:1] for a in uni], owners, out_form=1, expand="host")
    assert ext.shape == (1, P * N + 1)
    assert np.array_equal(ext[0], ref.extract(mk_rot_net_ref(ref, net, data, range(d))[0]).astype(np.int32))
    ck.close()
