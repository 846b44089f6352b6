"""Keys, inputs and the batch reference of tests/test_keyswitch_edges.py in one importable place (not collected by pytest, and it
never imports the engine).

Nothing of the keyswitch is restated here: `ks_batch` runs `Schoolbook._keyswitch` of tests/test_independent.py (keyswitch.jl:45-80 in
numpy int64) row by row, `mk_ks_batch` runs `MKSchoolbook.mk_keyswitch` (mk_internals.jl:397-411).  Added are

  Case / family      a stand-alone parameter set, and pick_ks_mode (csrc/engine_keys.hip) mirrored so that a test can state which
                     kernel family a (kN, t, gamma, ks_variant) can only get
  make_key           a synthetic key [kN][t][base-1][n+1]: uniform int32 words with the carry-chain words of signed_byte_plane planted
  make_inputs        uniform int32 rows [G][kN+1] with the fixed rows (all zero, rounded mask 0, every digit equal to d, rounding carries)
                     at the head of the batch and again at its tail, so that the ragged tile holds them
  boundary_rows      rows 0, 1, the last, and both rows either side of every sample-tile edge of a family
  ks_batch(mutant=)  the reference with ONE deliberate fault of a kernel emulated (MUTANTS below): the CPU self-checks require each of
                     them to change a word on the committed keys and inputs, which shows that these reach the edge the fault sits on
"""
import functools

import numpy as np

from test_independent import MKSchoolbook, Schoolbook, wrap32            # noqa: F401  (MKSchoolbook re-exported)

# words on which the balanced signed bytes of signed_byte_plane (csrc/kernels_keyswitch.hpp) carry: -128 bytes, carries that run through
# several planes, a carry that leaves the top plane, the two extremes
CARRY_WORDS = (0x80, 0x7f, 0x7fffff80, 0x80808080, 0x7f7f7f7f, 0xffffff80, 0x80000000, 0x7fffffff)

V4_SIZES = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 600)      # 32-sample A tile, 64-sample wave, 256-sample block, Gpad
V3_SIZES = (1, 15, 16, 17, 32, 33)                                              # 16-sample tile
V1_SIZES = (1, 3)                                                               # one workgroup per sample
TILE = {4: 32, 3: 16, 1: 1}                                                     # samples per tile of a family


def family(kN, t, gamma, variant=4):
    """pick_ks_mode (csrc/engine_keys.hip): the kernel family a key of kN mask words per party is laid out for under option ks_variant."""
    ok4 = gamma == 2 and t == 8 and kN % 128 == 0
    ok3 = gamma == 2 and t % 4 == 0 and kN % 16 == 0 and kN // 16 <= 128
    if variant == 4 and ok4:
        return 4
    if variant >= 3 and ok3:
        return 3
    return 1


class Case:
    """One stand-alone parameter set: (N, k, t, gamma, n), the ks_variant its engine is given and the batch sizes it runs."""

    def __init__(self, N, k, t, gamma, n, variant, sizes):
        self.N, self.k, self.t, self.gamma, self.n, self.variant, self.sizes = N, k, t, gamma, n, variant, tuple(sizes)
        self.kN, self.base = k * N, 1 << gamma
        self.family = family(self.kN, t, gamma, variant)
        self.name = f"v{self.family}-N{N}k{k}-t{t}g{gamma}-n{n}"
        self.seed = [N, k, t, gamma, n]                                          # (of the key and the inputs: the same for every variant)

    def with_variant(self, variant):
        return Case(self.N, self.k, self.t, self.gamma, self.n, variant, self.sizes)

    def __repr__(self):
        return self.name


V4_CASES = [Case(512, 1, 8, 2, 31, 4, V4_SIZES),      # n + 1 = 32: the b word is the last column of a full 32-word tile
            Case(512, 1, 8, 2, 32, 4, V4_SIZES),      # n + 1 = 33: the b word alone in a second tile
            Case(512, 1, 8, 2, 40, 4, V4_SIZES),
            Case(128, 1, 8, 2, 63, 4, V4_SIZES),      # kN % 512 != 0: the unsliced path
            Case(128, 3, 8, 2, 64, 4, V4_SIZES),      # unsliced, kN / 128 = 3 blocks of ks4_digits_kernel
            Case(512, 3, 8, 2, 5, 4, V4_SIZES)]       # sliced, 96 mask words per slice
V3_CASES = [Case(16, 3, 4, 2, 511, 3, V3_SIZES),      # 3 stages (odd); stride 512: exactly one chunk
            Case(16, 3, 4, 2, 512, 3, V3_SIZES),      # stride 516: one lane quad in a second chunk
            Case(64, 1, 12, 2, 6, 3, V3_SIZES),       # t / 4 = 3
            Case(2048, 1, 8, 2, 5, 3, V3_SIZES)] + [  # slice length 128, the LDS limit
            Case(512, 1, 8, 2, n, 3, V3_SIZES) for n in (8, 9, 10, 11)]          # every residue of (n + 1) % 4
V1_CASES = [Case(16, 1, 8, 2, n, 1, V1_SIZES) for n in (1022, 1023, 1024)] + [   # n + 1 = 1023, 1024, 1025 around the 1024-word chunk
            Case(16, 1, 31, 1, 255, 4, V1_SIZES),     # base 2, gamma t = 31 (the most tfhe_ctx_create takes): only the gather kernel takes it
            Case(16, 1, 31, 1, 256, 4, V1_SIZES),
            Case(64, 1, 6, 5, 7, 4, V1_SIZES),
            Case(64, 1, 1, 7, 7, 4, V1_SIZES)]
CASES = V4_CASES + V3_CASES + V1_CASES


# ---- keys ---------------------------------------------------------------------------------------------------------------------------
def planted_positions(case):
    """(i, j0) of the key rows that hold carry-chain words, with the offset each adds to the cycle over columns: mask words 0,
    kN/16 - 1, kN/16 (a v3 / v4 slice edge) and kN - 1, digit positions j = 1, 4, 5 and t (j0 = j - 1), those that exist, once each."""
    kN, t = case.kN, case.t
    iis = list(dict.fromkeys(i for i in (0, kN // 16 - 1, kN // 16, kN - 1) if 0 <= i < kN))
    jjs = list(dict.fromkeys(j - 1 for j in (1, 4, 5, t) if j <= t))
    return [(i, j0, a + b) for a, i in enumerate(iis) for b, j0 in enumerate(jjs)]


@functools.lru_cache(maxsize=None)
def _key(N, k, t, gamma, n):
    case = Case(N, k, t, gamma, n, 4, ())
    rng = np.random.default_rng([1] + case.seed)
    ks = rng.integers(-2**31, 2**31, size=(case.kN, t, case.base - 1, n + 1), dtype=np.int64)
    words = wrap32(np.array(CARRY_WORDS, np.int64))
    cols = np.arange(n + 1)
    for i, j0, off in planted_positions(case):
        ks[i, j0, :, :] = words[(cols + off) % 8]        # cycled over the output columns, column n - 1 and the b column n included
    ks = ks.astype(np.int32)
    ks.setflags(write=False)
    return ks


def make_key(case):
    """int32 [kN][t][base-1][n+1], read-only and shared: uniform words from a seeded generator, the eight CARRY_WORDS cycled over the
    columns of all base - 1 rows at planted_positions."""
    return _key(case.N, case.k, case.t, case.gamma, case.n)


def signed_byte_planes(v):
    """The four balanced signed bytes of 32-bit words, signed_byte_plane of csrc/kernels_keyswitch.hpp restated on int64 arrays:
    value == sum_p plane[p] 256^p (mod 2^32), every byte in [-128, 127]."""
    v = np.asarray(v, np.int64) & 0xffffffff
    planes = []
    for _ in range(4):
        u = v & 255
        s = np.where(u >= 128, u - 256, u)
        planes.append(s)
        v = ((v - s) & 0xffffffff) >> 8
    return planes


def _plane3_without_carry(words):
    """The words a key preparation would stand for if byte plane 3 were the word's own top byte, without the carry out of plane 2."""
    p = signed_byte_planes(words)
    raw = (np.asarray(words, np.int64) >> 24) & 255
    top = np.where(raw >= 128, raw - 256, raw)
    return wrap32(p[0] + (p[1] << 8) + (p[2] << 16) + (top << 24))


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def fixed_rows(case, rng):
    """The mask words [rows][kN] of the fixed rows after the all-zero one, in the order listed: rounded mask 0 (every digit zero), one row
    per digit value d whose rounded mask has every digit equal to d (the bits below the digits uniform), and 0x7fffffff, 0x80000000,
    2^(31 - gamma t) - 1 repeating (rounding carries into the top digit, a wrap, and the largest word that still rounds to digits 0)."""
    kN, t, gamma, base = case.kN, case.t, case.gamma, case.base
    low = 32 - gamma * t
    half = 1 << (low - 1)                                                        # keyswitch.jl:58: abar = a + 2^(31 - gamma t)
    rows = [np.full(kN, -half, np.int64)]
    for d in range(1, base):
        digits = sum(d << (32 - gamma * j) for j in range(1, t + 1))
        rows.append(digits + rng.integers(0, 1 << low, kN, dtype=np.int64) - half)
    rows.append(np.array([0x7fffffff, 0x80000000, half - 1], np.int64)[np.arange(kN) % 3])
    return wrap32(np.stack(rows))


@functools.lru_cache(maxsize=None)
def _inputs(N, k, t, gamma, n, G):
    case = Case(N, k, t, gamma, n, 4, ())
    rng = np.random.default_rng([2] + case.seed)
    x = rng.integers(-2**31, 2**31, size=(max(V4_SIZES), case.kN + 1), dtype=np.int64)[:G].copy()      # (row g the same at every G)
    fixed = fixed_rows(case, rng)
    x[0, :] = 0
    head = min(len(fixed), G - 1)
    x[1:1 + head, :case.kN] = fixed[:head]
    free = G - 1 - head                                   # rows beyond the head: the fixed rows again, at the end of the batch
    tail = min(len(fixed), free)
    if tail:
        x[G - tail:, :case.kN] = fixed[:tail]
    x = x.astype(np.int32)
    x.setflags(write=False)
    return x


def make_inputs(case, G):
    """int32 [G][kN+1], read-only and shared.  Row 0 is all zero, rows 1 .. take fixed_rows in their order (the b words stay uniform), and
    the last rows of the batch take them again where they do not fall on the head; as many as fit, in the order listed."""
    return _inputs(case.N, case.k, case.t, case.gamma, case.n, G)


def head_rows(case):
    """Number of rows at the head of a batch that are fixed: the zero row and fixed_rows."""
    return 1 + case.base + 1


def boundary_rows(fam, G):
    """Rows 0, 1, the last, and both rows either side of every multiple of the family's sample tile (v4: 32 samples per MFMA A tile,
    which holds the 64-sample wave, the 256-sample block and the padding to 64; v3: 16; v1 has one workgroup per sample)."""
    rows = {0, 1, G - 1}
    if TILE[fam] > 1:
        for b in range(TILE[fam], G, TILE[fam]):
            rows |= {b - 1, b}
    return sorted(r for r in rows if 0 <= r < G)


# ---- the batch reference and its mutants -------------------------------------------------------------------------------------------------
MUTANTS = ("drop_b", "last_slice", "second_half", "col", "plane3", "mux_const", "digit_t_high", "last_row")


@functools.lru_cache(maxsize=8)
def _schoolbook(N, k, t, gamma, n, mutated):
    case = Case(N, k, t, gamma, n, 4, ())
    ks = make_key(case)
    if mutated:
        ks = ks.astype(np.int64)
        for i, j0, _ in planted_positions(case):
            ks[i, j0] = _plane3_without_carry(ks[i, j0])
    return Schoolbook(n, N, k, 1, 1, t, gamma, np.zeros((n, 1, k + 1, k + 1, N), np.int8), ks=ks)


def schoolbook(case, plane3_mutant=False):
    """A Schoolbook (tests/test_independent.py) that holds only the case's synthetic keyswitch key."""
    return _schoolbook(case.N, case.k, case.t, case.gamma, case.n, bool(plane3_mutant))


def _keyswitch_digit_t_high(sb, u, kN):
    """Schoolbook._keyswitch with digit t read one position high (at digit t - 1's bits; above the word for t = 1)."""
    n, t, gamma = sb.n, sb.t, sb.gamma
    abar = wrap32(np.asarray(u[:kN], np.int64) + (1 << (32 - (1 + gamma * t))))
    shifts = 32 - gamma * np.arange(1, t + 1)
    shifts[-1] += gamma
    d = (abar[:, None] >> shifts) & ((1 << gamma) - 1)
    i, j = np.nonzero(d)
    res = -sb.ks[i, j, d[i, j] - 1].sum(axis=0)
    res[n] += u[kN]
    return wrap32(res)


def ks_batch(case, x, x1=None, two=None, rows=None, mutant=None, arg=None):
    """The keyswitch of rows x [G][kN+1] under make_key(case), int32 [len(rows)][n+1] (rows None: all): Schoolbook._keyswitch per row.
    Row g with two[g] set is the two-operand form of a MUX gate (gates.jl:174): x[g] + x1[g] word by word, plus 2^29 on the b word.

    `mutant` emulates one kernel fault (arg: its parameter):
      drop_b        the b word is not added for rows of the last group of `arg` samples (rows >= ((G - 1) // arg) arg)
      last_slice    the last kN/16 mask words contribute nothing
      second_half   for G > 512, the second half of the mask words contributes nothing
      col           output column `arg` keeps what it was initialised to (0, or the b word in column n)
      plane3        the planted key words are taken with byte plane 3 lacking the carry from plane 2
      mux_const     2^29 is not added on two-operand rows
      digit_t_high  digit t is read one digit position high
      last_row      the last row of the batch is not computed (all zero)"""
    assert mutant is None or mutant in MUTANTS, mutant
    x = np.asarray(x, np.int64)
    G, kN, n = x.shape[0], case.kN, case.n
    rows = range(G) if rows is None else rows
    sb = schoolbook(case, mutant == "plane3")
    silent = -(1 << (31 - case.gamma * case.t))           # a mask word whose rounded form is 0: it selects no key row
    out = np.zeros((len(rows), n + 1), np.int64)
    for r, g in enumerate(rows):
        u = x[g].copy()
        if two is not None and two[g]:
            u = wrap32(u + np.asarray(x1[g], np.int64))
            if mutant != "mux_const":
                u[kN] = wrap32(u[kN] + 2**29)
        if mutant == "last_row" and g == G - 1:
            continue
        if mutant == "drop_b" and g >= (G - 1) // arg * arg:
            u[kN] = 0
        if mutant == "last_slice":
            u[kN - kN // 16:kN] = silent
        if mutant == "second_half" and G > 512:
            u[kN // 2:kN] = silent
        res = _keyswitch_digit_t_high(sb, u, kN) if mutant == "digit_t_high" else sb._keyswitch(u, sb.ks, kN)
        if mutant == "col":
            res[arg] = u[kN] if arg == n else 0
        out[r] = res
    return out.astype(np.int32)


def mutants_of(case, G):
    """The (mutant, arg) pairs that apply to a stand-alone batch of G rows of `case`, from how make_inputs lays the rows out: row 0 is
    all zero and row 1 has every digit zero, so a fault in a b word needs G >= 2 and one in a key contribution G >= 3 (row 2 has every
    digit 1 and reads all of the key's rows for d = 1, the planted ones among them); rows 2 .. base and the carry row have equal digits
    at positions t - 1 and t, so digit_t_high needs a uniform row, G > 2 head_rows - 1 (or t = 1, where it reads above the word)."""
    out = []
    if G >= 2:
        groups = {4: (32, 64, 256), 3: (16,), 1: (1,)}[case.family]
        out += [("drop_b", g) for g in groups] + [("last_row", None)]
    if G >= 3:
        out += [("last_slice", None), ("col", case.n - 1), ("col", case.n)]
        if case.gamma == 2 and case.t == 8 and case.kN % 128 == 0:              # a key that ks4_prepare_kernel can be given
            out.append(("plane3", None))
    if G > 512:
        out.append(("second_half", None))
    if G >= 2 * head_rows(case) or (case.t == 1 and G >= 3):
        out.append(("digit_t_high", None))
    return out


def mk_ks_batch(msb, ext_rows):
    """MKSchoolbook.mk_keyswitch (mk_internals.jl:397-411) over extracted rows [...][P N + 1]: int32 [...][P n + 1]."""
    ext = np.asarray(ext_rows, np.int64)
    flat = ext.reshape(-1, ext.shape[-1])
    out = np.stack([msb.mk_keyswitch(u) for u in flat]).astype(np.int32)
    return out.reshape(ext.shape[:-1] + (out.shape[-1],))
