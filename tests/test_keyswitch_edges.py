"""The three keyswitch kernel families (csrc/kernels_keyswitch.hpp: v4 int8 MFMA, v3 tiled integer VALU, v1 gather) at the tile, slice
and batch edges their launcher (launch_keyswitch, csrc/engine_dispatch.hip) decides on.  The keyswitch is exact integer arithmetic:
every comparison is word-for-word equality, with the C oracle (Oracle.keyswitch / gates / mk_gate_nand) on every row and with the integer
restatements of tests/test_independent.py (Schoolbook._keyswitch, schoolbook_gate, MKSchoolbook.mk_keyswitch) on rows 0, 1, the last
and both rows either side of every sample-tile edge of the family (keyswitch_ref.boundary_rows).

Stand-alone cases need no key generation: tfhe_load_keyswitch_key takes any int32 [kN][t][base-1][n+1] and tfhe_keyswitch_batch needs no
bootstrapping key.  The keys are uniform words with the carry-chain words of signed_byte_plane planted (keyswitch_ref.make_key), the
inputs uniform rows with fixed rows at the head and the tail of the batch (make_inputs).  Each family is pinned by its parameters:
keyswitch_ref.family mirrors pick_ks_mode, and every case states the family its (kN, t, gamma, ks_variant) can only get.

  v4   (kN, n) = (512, 31) (512, 32) (512, 40): n + 1 = 32 / 33 around the 32-word tile; (128, 63) (384, 64): kN % 512 != 0, the unsliced
       path, one and three blocks of ks4_digits_kernel; (1536, 5): sliced, 96 mask words per slice.  G = 1 ... 600 over the 32-sample A
       tile, the 64-sample wave, the 256-sample block, the padding to 64 and the switch from 16 slices to option ks_slices at G = 513;
       G = 513, 600 at kN = 512 with ks_slices = 1 (direct stores), 2 and 4 (atomics on the pre-initialised output)
  v3   (kN, t, n) = (48, 4, 511) (48, 4, 512): three stages, one 512-word chunk and one lane quad more; (64, 12, 6): t / 4 = 3;
       (2048, 8, 5): slice length 128; (512, 8, 8 ... 11): every residue of the 4-word row padding.  G = 1 ... 33 over the 16-sample tile
  v1   n + 1 = 1023, 1024, 1025 around the 1024-word chunk; base 2 with gamma t = 31; base 32; base 128 with t = 1
  cross-family: the v3 and v1 engines on every v4 key and batch give the v4 words

Two operands (MUX: e1, 2^29), scattered outputs (dst) and chained b words (parties after the first, add_b = 0) exist only behind a
rotation and so run on real keys, N = 128 with 6 CMUX steps per rotation (4 per party under a multi-key key): gate batches of 17, 65
and 513 with every third gate a MUX and NOT / COPY / CONST1 among the others, the same gates as one gates_level onto output wires in
reverse and in permuted order, and mk_gate_nand of 17, 65 and (v4) 257 rows for two and three parties, on all three families.

CPU self-checks (no GPU): on the keys and inputs of every stand-alone case the batch reference equals Oracle.keyswitch on all rows, and
each mutant of keyswitch_ref.ks_batch - one emulated kernel fault - changes a word wherever it applies (keyswitch_ref.mutants_of), so
the committed seeds reach the edge the fault sits on:

  drop_b (16 / 32, 64, 256 / 1)   the b word of the rows in the last (ragged) v3 tile / v4 A tile, wave, block / v1 workgroup
  last_slice                      the last of the 16 mask-word slices of v3 and sliced v4 (planted mask words kN/16 - 1, kN/16, kN - 1)
  second_half                     the second blockIdx.z of v4 at G > 512 with ks_slices = 2
  col n - 1, col n                the last word tile (v4: 32 words), lane quad and chunk (v3: 4, 512), chunk (v1: 1024); the b column
  plane3                          the carry from byte plane 2 into plane 3 in ks4_prepare_kernel, on the planted words alone
  mux_const                       2^29 on two-operand rows (the e1 path of all three families and of ks3_init_kernel)
  digit_t_high                    the bit position of digit t (v4: the shift 27 - 2 (4 h + q); v3: pos; v1: 32 - j gamma)
  last_row                        the last row of the batch (the clamps min(g, G - 1) and the guards gg < G)
"""
import functools

import numpy as np
import pytest

import keyswitch_ref as R
from keyswitch_ref import CASES, V1_CASES, V3_CASES, V4_CASES

MU = 2**29
ids = lambda cases: [c.name for c in cases]                                   # noqa: E731


def _oracle(orc, case):
    o = orc.Oracle(case.n, case.N, case.k, 1, 1, case.t, case.gamma)
    o.load_keyswitch_key(R.make_key(case))
    return o


@functools.lru_cache(maxsize=None)
def _want_cached(orc, N, k, t, gamma, n, G):
    case = R.Case(N, k, t, gamma, n, 4, ())
    want = _oracle(orc, case).keyswitch(R.make_inputs(case, G))
    want.setflags(write=False)
    return want


def _want(orc, case, G):
    """Oracle.keyswitch of the case's batch of G rows: computed once, shared by every test and family, read-only."""
    return _want_cached(orc, case.N, case.k, case.t, case.gamma, case.n, G)


# ---- CPU self-checks of the tests -----------------------------------------------------------------------------------------------------
def test_each_family_is_pinned_by_its_parameters():
    """pick_ks_mode mirrored: the v4 cases can only get v4 at the default ks_variant and v3 / v1 at ks_variant 3 / 1 (the cross-family
    engines); the v3 cases only v3 at ks_variant 3; the v1 cases only v1 - by ks_variant 1 at base 4, by their base or length under the
    default.  The shapes are the ones the edges need."""
    for c in V4_CASES:
        assert (c.family, c.with_variant(3).family, c.with_variant(1).family) == (4, 3, 1), c
        assert c.gamma == 2 and c.t == 8 and c.kN % 128 == 0
    assert [(c.kN, c.n) for c in V4_CASES] == [(512, 31), (512, 32), (512, 40), (128, 63), (384, 64), (1536, 5)]
    assert [c.kN % 512 == 0 for c in V4_CASES] == [True, True, True, False, False, True]          # sliced / unsliced
    for c in V3_CASES:
        assert c.family == 3 and c.variant == 3 and c.kN // 16 <= 128, c
    assert [(c.kN, c.t, c.n) for c in V3_CASES] == [(48, 4, 511), (48, 4, 512), (64, 12, 6), (2048, 8, 5)] + [(512, 8, n) for n in (8, 9, 10, 11)]
    assert (V3_CASES[0].kN // 16) * (V3_CASES[0].t // 4) == 3 and V3_CASES[3].kN // 16 == 128       # odd stage count; the slice limit
    for c in V1_CASES:
        assert c.family == 1, c
        assert c.variant == 1 or all(R.family(c.kN, c.t, c.gamma, v) == 1 for v in (4, 3, 1)), c
        assert c.gamma * c.t <= 31
    assert [(c.N, c.t, c.gamma, c.n) for c in V1_CASES] == [(16, 8, 2, 1022), (16, 8, 2, 1023), (16, 8, 2, 1024), (16, 31, 1, 255),
                                                            (16, 31, 1, 256), (64, 6, 5, 7), (64, 1, 7, 7)]


def test_carry_words_are_planted_where_stated():
    """Every key holds all eight carry-chain words, in all base - 1 rows of digit positions 1, 4, 5, t of mask words 0, kN/16 - 1, kN/16,
    kN - 1 (those that exist), also in columns n - 1 and n, and is a few MB at most; the balanced bytes of these words sum back to them, lie
    in [-128, 127] and, for five of the eight, differ from the word's plain bytes in plane 3 or below (a carry took place)."""
    words = R.wrap32(np.array(R.CARRY_WORDS, np.int64))
    planes = R.signed_byte_planes(words)
    assert np.array_equal(R.wrap32(sum(p << (8 * i) for i, p in enumerate(planes))), words)
    assert all(((p >= -128) & (p <= 127)).all() for p in planes)
    assert [int(p) for p in planes[3]] == [0, 0, -128, -127, 127, 0, -128, -128]
    assert int((R._plane3_without_carry(words) != words).sum()) == 4                 # 0x7fffff80, 0x80808080, 0xffffff80, 0x7fffffff
    for c in CASES:
        ks = R.make_key(c)
        assert ks.shape == (c.kN, c.t, c.base - 1, c.n + 1) and ks.dtype == np.int32 and ks.nbytes <= 4 << 20, c
        pos = R.planted_positions(c)
        assert {i for i, _, _ in pos} == {i for i in (0, c.kN // 16 - 1, c.kN // 16, c.kN - 1) if i >= 0}, c
        assert {j + 1 for _, j, _ in pos} == {j for j in (1, 4, 5, c.t) if j <= c.t}, c
        for i, j0, off in pos:
            assert np.array_equal(ks[i, j0, 0], words[(np.arange(c.n + 1) + off) % 8]), (c, i, j0)      # columns n - 1 and n included
            assert (ks[i, j0] == ks[i, j0, :1]).all()                                # all base - 1 rows alike
        assert set(np.unique(np.concatenate([ks[i, j0, 0] for i, j0, _ in pos])).tolist()) == set(words.tolist()), c


def test_fixed_rows_have_the_stated_digits():
    """Row 0 is zero, row 1 rounds to 0, rows 2 ... have every digit equal to d = 1 ... base - 1, the next row carries into the top digit;
    the tail of the batch holds the same rows where it does not fall on the head, so the ragged tile has them."""
    for c in CASES:
        G = max(c.sizes)
        x = R.make_inputs(c, G).astype(np.int64)
        assert x.shape == (G, c.kN + 1)
        assert not x[0].any()
        half = 1 << (31 - c.gamma * c.t)
        digits = lambda row: (R.wrap32(row[:c.kN] + half)[:, None] >> (32 - c.gamma * np.arange(1, c.t + 1))) & (c.base - 1)   # noqa: E731
        if G >= 2:
            assert not R.wrap32(x[1, :c.kN] + half).any()
        for d in range(1, c.base):
            if 1 + d < G:
                assert (digits(x[1 + d]) == d).all(), (c, d)
        if G >= 2 * R.head_rows(c):
            carry = digits(x[c.base + 1])
            assert (carry[0::3, 0] == c.base >> 1).all() and not carry[:, 1:].any()   # 0x7fffffff + 2^(31 - gamma t) wraps to 0x80000000 + ...
            for back, d in zip(range(2, c.base + 1), range(c.base - 1, 0, -1)):
                assert (digits(x[G - back]) == d).all(), (c, d)
            assert np.array_equal(x[G - 1, :c.kN], x[c.base + 1, :c.kN])
            assert len(np.unique(digits(x[R.head_rows(c)]))) == c.base              # a uniform row between head and tail
    assert R.boundary_rows(4, 600) == sorted({0, 1, 599} | {b - e for b in range(32, 600, 32) for e in (0, 1)})
    assert R.boundary_rows(3, 33) == [0, 1, 15, 16, 31, 32] and R.boundary_rows(1, 3) == [0, 1, 2] and R.boundary_rows(4, 1) == [0]


@pytest.mark.parametrize("case", CASES, ids=ids(CASES))
def test_reference_equals_oracle_and_every_mutant_differs(orc, case):
    """On the key and the inputs of the case, at every batch size: the batch schoolbook equals Oracle.keyswitch on all rows, and every
    mutant that applies (keyswitch_ref.mutants_of) changes at least one word of the rows it is evaluated on - the fixed rows at head and
    tail, the boundary rows and the first uniform rows."""
    for G in case.sizes:
        x = R.make_inputs(case, G)
        want = _want(orc, case, G)
        assert np.array_equal(R.ks_batch(case, x), want), (case, G)
        rows = sorted(set(R.boundary_rows(case.family, G)) | set(range(min(G, 2 * R.head_rows(case) + 1))) | set(range(max(0, G - R.head_rows(case)), G)))
        for mutant, arg in R.mutants_of(case, G):
            assert not np.array_equal(R.ks_batch(case, x, rows=rows, mutant=mutant, arg=arg), want[rows]), (case, G, mutant, arg)
    applied = {m for G in case.sizes for m, _ in R.mutants_of(case, G)}
    expect = {"drop_b", "last_row", "last_slice", "col"} | ({"second_half"} if case.family == 4 else set())
    expect |= {"plane3"} if R.family(case.kN, case.t, case.gamma) == 4 else set()      # (a key v4 could be given, whoever serves it here)
    expect |= {"digit_t_high"} if case.family != 1 or case.t == 1 else set()            # (v1's batches of 3 hold no uniform row)
    assert applied == expect, (case, applied)


def test_two_operand_reference_and_its_mutant(orc):
    """The two-operand form of ks_batch (MUX rows: x + x1 word by word, 2^29 on the b word, gates.jl:174) against Oracle.keyswitch of
    the rows summed here; omitting 2^29 changes exactly the b words of the two-operand rows."""
    case, G = V4_CASES[3], 33
    x = R.make_inputs(case, G)
    x1 = np.random.default_rng(29).integers(-2**31, 2**31, size=x.shape, dtype=np.int64).astype(np.int32)
    two = np.arange(G) % 3 == 2
    summed = x.astype(np.int64) + np.where(two[:, None], x1.astype(np.int64), 0)
    summed[two, case.kN] += MU
    want = _oracle(orc, case).keyswitch(R.wrap32(summed).astype(np.int32))
    assert np.array_equal(R.ks_batch(case, x, x1, two), want)
    diff = R.ks_batch(case, x, x1, two, mutant="mux_const") != want
    assert np.array_equal(diff.any(axis=1), two) and not diff[:, :case.n].any()


# ---- stand-alone cases on the GPU --------------------------------------------------------------------------------------------------------
def _engine(tfhe, case):
    """An engine with the case's ks_variant chosen before its synthetic key is loaded (no bootstrapping key)."""
    p = tfhe.SchemeParameters(case.n, 0.0, case.N, case.k, 2, 8, 0.0, case.t, case.gamma, 0.0, 1)
    eng = tfhe.Engine(p, 0)
    eng.set_option("ks_variant", case.variant)
    eng.load_keyswitch_key(R.make_key(case))
    return eng


def _check_batch(eng, orc, case, G, what=""):
    x = R.make_inputs(case, G)
    got = eng.keyswitch(x)
    assert np.array_equal(got, _want(orc, case, G)), (case, G, what)
    rows = R.boundary_rows(case.family, G)
    assert np.array_equal(got[rows], R.ks_batch(case, x, rows=rows)), (case, G, what, "schoolbook")
    if G == 1:      # (row 0 is all zero and so is its result: a batch of one also with a row that reads the key, the last of the largest batch)
        big = max(case.sizes)
        assert np.array_equal(eng.keyswitch(R.make_inputs(case, big)[-1:]), _want(orc, case, big)[-1:]), (case, "one non-zero row")
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("case", V4_CASES, ids=ids(V4_CASES))
def test_v4_sample_tiles_word_tiles_and_slices(tfhe, orc, case):
    """keyswitch_kernel_v4 behind ks4_digits_kernel (and ks3_init_kernel where the mask words are sliced) on one engine, G over every
    sample-tile edge; where kN = 512, G = 513 and 600 under ks_slices 1, 2 and 4: the same words from direct stores and from atomics."""
    assert case.family == 4
    eng = _engine(tfhe, case)
    try:
        assert eng.get_option("ks_variant") == 4 and eng.get_option("ks_slices") == 2
        for G in case.sizes:
            got = _check_batch(eng, orc, case, G)
            if case.kN == 512 and G > 512:
                for slices in (1, 4, 2):
                    eng.set_option("ks_slices", slices)
                    assert np.array_equal(_check_batch(eng, orc, case, G, f"ks_slices = {slices}"), got), (case, G, slices)
    finally:
        eng.close()


@pytest.mark.gpu
def test_ks_slices_takes_1_2_4_only(tfhe):
    eng = _engine(tfhe, V4_CASES[0])
    try:
        for bad in (3, 0, 8):
            with pytest.raises(tfhe.EngineError):
                eng.set_option("ks_slices", bad)
        assert eng.get_option("ks_slices") == 2
        for ok in (1, 4, 2):
            eng.set_option("ks_slices", ok)
            assert eng.get_option("ks_slices") == ok
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", V3_CASES, ids=ids(V3_CASES))
def test_v3_tiles_stages_and_row_padding(tfhe, orc, case):
    """keyswitch_kernel_v3 behind ks3_init_kernel in single-key mode: a full 16-sample tile plus a ragged one, an odd stage count, t = 4
    and 12, the slice length 128, the 4-word row padding at every residue and the 512-word chunk edge."""
    assert case.family == 3
    eng = _engine(tfhe, case)
    try:
        assert eng.get_option("ks_variant") == 3
        for G in case.sizes:
            _check_batch(eng, orc, case, G)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", V1_CASES, ids=ids(V1_CASES))
def test_v1_chunk_edge_and_any_base(tfhe, orc, case):
    """keyswitch_kernel (gather): n + 1 around its 1024-word chunk, base 2 at the longest decomposition a context takes, base 32, base 128
    with a single digit."""
    assert case.family == 1
    eng = _engine(tfhe, case)
    try:
        for G in case.sizes:
            _check_batch(eng, orc, case, G)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [3, 1])
@pytest.mark.parametrize("case", V4_CASES, ids=ids(V4_CASES))
def test_v3_and_v1_give_the_v4_words(tfhe, orc, case, variant):
    """Every (kN, n) v4 accepts, on the same key and the same batches, through the v3 and the v1 engine (ks_variant chosen before the
    key load): the oracle's words, which are what test_v4_sample_tiles_word_tiles_and_slices requires of v4."""
    other = case.with_variant(variant)
    assert other.family == variant
    eng = _engine(tfhe, other)
    try:
        assert eng.get_option("ks_variant") == variant
        for G in other.sizes:
            _check_batch(eng, orc, other, G)
    finally:
        eng.close()


# ---- two operands, scattered outputs, chained b words: real keys behind a rotation ---------------------------------------------------------
GATE_SIZES = (17, 65, 513)
_OTHERS = ("NAND", "NOT", "XOR", "COPY", "AND", "CONST1", "ORYN", "XNOR")


def _gate_names(B):
    """Every third gate a MUX; NOT, COPY and CONST1 among the others, so that fewer than B samples reach the keyswitch."""
    return ["MUX" if g % 3 == 2 else _OTHERS[(g - g // 3) % len(_OTHERS)] for g in range(B)]


@pytest.fixture(scope="module")
def gate_set(tfhe, orc):
    """N = 128, k = 1, n = 6 (v4 by default, v3 and v1 by ks_variant): keys, the operands of the largest batch - even rows encryptions,
    odd rows arbitrary words - and Oracle.gates of every batch size, computed once."""
    from test_any_params import _setup
    K = _setup(tfhe, orc, 6, 128, 1, 3, 6)
    rng = np.random.default_rng(128)
    B = max(GATE_SIZES)
    ins = []
    for _ in range(3):
        v = rng.integers(-2**31, 2**31, size=(B, 7), dtype=np.int64).astype(np.int32)
        v[0::2] = tfhe.encrypt(K.rng, K.sk, rng.integers(0, 2, (B + 1) // 2).astype(bool)).data
        ins.append(v)
    want = {}
    for B in GATE_SIZES:
        ops = np.array([tfhe.OPCODES[nm] for nm in _gate_names(B)], np.uint8)
        want[B] = K.oracle.gates(ops, *[v[:B] for v in ins], nthreads=8)
    yield K, ins, want
    K.ck.close()


def test_gate_mix_reaches_fewer_keyswitches_than_gates():
    for B in GATE_SIZES:
        names = _gate_names(B)
        assert names.count("MUX") == B // 3 and {"NOT", "COPY", "CONST1"} <= set(names)
        assert 0 < sum(nm not in ("NOT", "COPY", "CONST1") for nm in names) < B
    ks = sum(nm not in ("NOT", "COPY", "CONST1") for nm in _gate_names(513))
    assert ks > 256                                                               # more than one v4 block, several v3 tiles


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [4, 3, 1])
def test_gates_batch_and_level_through_each_family(tfhe, gate_set, variant):
    """Engine.gates on 17, 65 and 513 mixed gates (the keyswitch takes e0, e1 and dst from the gate plan) against Oracle.gates on every row
    and schoolbook_gate on the gates whose keyswitch sample sits at a tile edge; then the same gates as one gates_level on a wire table
    whose output wires run in reverse and in a seeded permutation: row for row the batch's words."""
    from test_independent import Schoolbook, schoolbook_gate
    K, ins, want = gate_set
    p = K.params
    assert R.family(128, 8, 2, variant) == variant
    eng = tfhe.Engine(p, 0)
    try:
        eng.set_option("ks_variant", variant)
        eng.load_bootstrap_key(K.ck.bootstrap_key)
        eng.load_keyswitch_key(K.ck.keyswitch_key)
        sb = Schoolbook(6, 128, 1, 3, 6, 8, 2, K.ck.bootstrap_key, K.ck.keyswitch_key)
        for B in GATE_SIZES:
            names = _gate_names(B)
            ops = np.array([tfhe.OPCODES[nm] for nm in names], np.uint8)
            x, y, z = (v[:B] for v in ins)
            got = eng.gates(ops, x, y, z)
            assert np.array_equal(got, want[B]), (variant, B)
            sample = np.cumsum([nm not in ("NOT", "COPY", "CONST1") for nm in names]) - 1      # keyswitch sample of a bootstrapped gate
            edge = set(R.boundary_rows(3, int(sample[-1]) + 1))                                 # multiples of 16 hold those of 32, 64, 256
            for g in [g for g in range(B) if int(sample[g]) in edge or g in (0, 1, B - 1)]:
                assert np.array_equal(got[g], schoolbook_gate(sb, names[g], x[g], y[g], z[g]).astype(np.int32)), (variant, B, g, names[g])
            idx = np.arange(B, dtype=np.int32)
            eng.wires_alloc(4 * B)
            eng.wires_upload(0, np.concatenate([x, y, z]))
            for order in (idx[::-1].copy(), np.random.default_rng(B).permutation(B).astype(np.int32)):
                eng.wires_upload(3 * B, np.zeros((B, 7), np.int32))
                eng.gates_level(ops, idx, idx + B, idx + 2 * B, 3 * B + order)
                assert np.array_equal(eng.wires_download(3 * B, B)[order], got), (variant, B)
    finally:
        eng.close()


MK_SIZES = (17, 65, 257)


@functools.lru_cache(maxsize=None)
def _mk_set(tfhe, orc, parties):
    """_mk of tests/test_any_params.py with N = 128 (pick_ks_mode gives a multi-key key of N = 128 mask words per party v4 by default),
    n = 4, l = 4, beta = 5; operands of 257 rows, even rows encryptions, odd rows arbitrary words; Oracle.mk_gate_nand once per size."""
    from test_any_params import _mk, _mk_oracle
    n = 4
    p, rng, sks, ck = _mk(tfhe, orc, parties, 128, 4, 5, n, seed=128)
    B = max(MK_SIZES)
    ins = []
    for _ in range(2):
        v = rng.integers(-2**31, 2**31, size=(B, parties * n + 1), dtype=np.int64).astype(np.int32)
        v[0::2] = tfhe.mk_encrypt(rng, sks, rng.integers(0, 2, (B + 1) // 2).astype(bool))
        ins.append(v)
    o = _mk_oracle(orc, p, parties, ck)
    want = {B: o.mk_gate_nand(ins[0][:B], ins[1][:B], nthreads=8) for B in MK_SIZES}
    msb = R.MKSchoolbook(n, 128, 4, 5, 8, 2, parties, ck.bootstrap_key, ck.keyswitch_key)
    msb.extracted = {}                                    # row -> its schoolbook rotation (row g is the same at every batch size)
    return p, ck, ins, want, msb


def _mk_schoolbook_rows(msb, x, y, rows):
    """mk_gate_nand (mk_gates.jl:7-12) of the given rows in integers: the schoolbook rotation (once per row), then
    MKSchoolbook.mk_keyswitch."""
    w = msb.P * msb.n
    for g in rows:
        if g not in msb.extracted:
            t = R.wrap32(-x[g].astype(np.int64) - y[g].astype(np.int64))
            t[w] = R.wrap32(t[w] + MU)
            msb.extracted[g] = msb.mk_bootstrap_wo_keyswitch(MU, t)
    return R.mk_ks_batch(msb, np.stack([msb.extracted[g] for g in rows]))


@pytest.mark.parametrize("parties", [2, 3])
def test_mk_boundary_reference_equals_oracle(tfhe, orc, parties):
    """CPU: the multi-key schoolbook rows that the GPU test compares with equal Oracle.mk_gate_nand at the edge rows of a 65-row batch."""
    p, ck, ins, want, msb = _mk_set(tfhe, orc, parties)
    assert R.family(128, 8, 2, 4) == 4
    rows = R.boundary_rows(4, 65)
    assert np.array_equal(_mk_schoolbook_rows(msb, ins[0], ins[1], rows), want[65][rows])


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [4, 3, 1])
@pytest.mark.parametrize("parties", [2, 3])
def test_mk_gate_nand_chains_the_b_word_through_each_family(tfhe, orc, parties, variant):
    """mk_gate_nand under a multi-key key of N = 128 (the _mk builder of test_any_params.py; N = 128 already gives v4): one keyswitch
    launch per party, the parties after the first accumulating into the b word the first one wrote (add_b = 0).  17 and 65 rows on all
    three families, 257 rows - two v4 blocks - on v4; Oracle.mk_gate_nand on every row, MKSchoolbook.mk_keyswitch behind a schoolbook
    rotation on the rows at the tile edges."""
    p, ck, ins, want, msb = _mk_set(tfhe, orc, parties)
    assert R.family(128, 8, 2, variant) == variant
    eng = tfhe.Engine(p, 0)
    try:
        eng.set_option("ks_variant", variant)
        eng.mk_load_bootstrap_key(ck.bootstrap_key, parties)
        eng.mk_load_keyswitch_key(ck.keyswitch_key, parties)
        for B in MK_SIZES if variant == 4 else MK_SIZES[:2]:
            x, y = ins[0][:B], ins[1][:B]
            got = eng.mk_gate_nand(x, y)
            assert np.array_equal(got, want[B]), (parties, variant, B)
            rows = R.boundary_rows(variant, B)
            assert np.array_equal(got[rows], _mk_schoolbook_rows(msb, x, y, rows)), (parties, variant, B, "schoolbook")
    finally:
        eng.close()
