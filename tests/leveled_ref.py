"""The integer references of leveled mode in one importable place (not collected by pytest: tests/fuzz_leveled.py and
tests/test_leveled_fuzz.py import it, and so do the form-2 comparisons of test_leveled / test_cmux_net / test_rot_net).

Nothing is copied: `Schoolbook`, `monomial`, `wrap32` come from test_independent.py, `Tree` from test_leveled.py, `MKTree` and `Setup` from
test_mk_leveled.py, `rot_net_ref` from test_rot_net.py.  Added here is only what was missing:

  net_ref            rot_net_ref with every rotation 0, for a plain CmuxNet, over a Tree or an MKTree
  ks_ref             the integer keyswitch (keyswitch.jl:45-80, Schoolbook.keyswitch) over rows, from ck.keyswitch_key
  trivial_selectors  the noiseless, zero-mask TGSW sample of a bit (and mk_trivial_selectors, its expanded multi-key form)
  known_tree / known_net / known_rot_net / extract0: the closed-form known answer below, in which no schoolbook takes part

The known answer.  A trivial selector of the bit b holds b g_p (g_p = 2^(32 - p beta), tgsw.jl:8-21) on coefficient 0 of the diagonal
polynomials [p][j][j] and zeros elsewhere, so C (.) d = sum_p digit_p(d) b g_p = b (d - (d mod h)) with h = 2^(32 - l beta): decompose
(tgsw.jl:99-117) floors.  On samples whose words are all multiples of h (a rotation and a wrapping difference keep them so) a CMUX
d0 + C (.) (d1 - d0) is therefore exactly d0 (b = 0) or d1 (b = 1), and a whole network returns exactly the (rotated) entry that
CmuxNet.evaluate_clear / RotNet.evaluate_clear select on the plain words.  The multi-key form: a party with zero key material (s = 0,
r = 0, no noise, c1 = f1 = 0, public keys 0) uni-encrypts b as c0 = d1 = b g (constant term), d0 = f0 = 0 (mk_internals.jl:185-227), and
RGSW.Expand (:304-345) of that is x = 0, y[p][party] = b g_p, c0[p] = b g_p, c1 = 0 in the layout x | y | c0 | c1 (:243-271); in
mk_tgsw_extern_mul (:348-391) mask i reads y[.][party] with the digits of a_i and the body reads c0 with the digits of b: the same
b (d - (d mod h)) on every polynomial.

Float64.  Every row of such a selector has ONE non-zero key coefficient, so a coefficient of a product is a single term digit g_p,
|digit g_p| <= 2^(beta-1) 2^(32-beta) = 2^31, and the sum over the l rows that feed one output polynomial is d - (d mod h), at most
2^32 in magnitude (the other (k+1) l - l or l P products are zero): 21 bits below the 2^53 of a Float64 at ANY (N, k, l, beta), also
at the sets of exactness class 0.  That is why the known answer is the part of the fuzz that no set skips.
tests/test_leveled_fuzz.py::test_known_answer_stays_inside_float64 computes exactly these products with a complex128 numpy.fft
negacyclic transform at the largest pinned and fuzzed sets and records the worst distance from an integer (profiles/leveled_fuzz.txt).
"""
import numpy as np

from test_independent import Schoolbook, monomial, wrap32            # noqa: F401  (re-exported)
from test_leveled import Tree                                        # noqa: F401
from test_mk_leveled import MKTree, Setup                            # noqa: F401
from test_rot_net import rot_net_ref                                 # noqa: F401


class _ZeroRotations:
    """A CmuxNet seen as a RotNet whose rotations are all 0: records (src0, src1, var, 0, 0)."""

    def __init__(self, net, N):
        self.net, self.levels, self.degree = net, net.levels, N

    def level(self, v):
        lv = np.asarray(self.net.level(v))[:, :3]
        return np.concatenate([lv, np.zeros((len(lv), 2), lv.dtype)], axis=1)


def net_ref(ref, net, table, sels):
    """The schoolbook network of a plain CmuxNet: rot_net_ref with zero rotations.  `ref` is a Tree (table [E][k+1][N]) or an MKTree
    ([E][P+1][N]); sels[var] is the selector behind each variable of the row.  Returns the last level, int64 [F][polys][N]."""
    return rot_net_ref(ref, _ZeroRotations(net, ref.N), table, sels)


def ks_schoolbook(params, keyswitch_key):
    """A Schoolbook that holds only the keyswitch key of a single-key cloud key (int32 [k N][t][2^gamma - 1][n + 1])."""
    p = params
    return Schoolbook(p.lwe_size, p.tlwe_polynomial_degree, p.tlwe_mask_size, p.bs_decomp_length, p.bs_log2_base, p.ks_decomp_length, p.ks_log2_base,
                      np.zeros((p.lwe_size, p.bs_decomp_length, p.tlwe_mask_size + 1, p.tlwe_mask_size + 1, p.tlwe_polynomial_degree), np.int8),
                      ks=keyswitch_key)


def ks_ref(sb, ext_rows):
    """The integer keyswitch (keyswitch.jl:45-80; Schoolbook.keyswitch) of extracted samples [...][k N + 1]: int32 [...][n + 1].  `sb` is a
    Schoolbook with the cloud key's keyswitch key (ks_schoolbook(params, ck.keyswitch_key)); the engine takes no part."""
    ext = np.asarray(ext_rows)
    flat = ext.reshape(-1, ext.shape[-1]).astype(np.int64)
    out = np.stack([sb.keyswitch(u) for u in flat]).astype(np.int32)
    return out.reshape(ext.shape[:-1] + (sb.n + 1,))


def gadget_h(l, beta):
    """h = 2^(32 - l beta): what the gadget decomposition cuts off."""
    return 1 << (32 - l * beta)


def multiples_of_h(words, l, beta):
    """Int32 words with the bits below h cleared."""
    return (np.asarray(words, np.int64) & ~np.int64(gadget_h(l, beta) - 1)).astype(np.int32)


def trivial_selectors(bits, N, k, l, beta):
    """The noiseless, zero-mask TGSW sample of each bit b: int32 [S][l][k+1][k+1][N] with [s, p, j, j, 0] = b 2^(32 - (p + 1) beta) (as a
    32-bit word: 2^31 is -2^31) and everything else 0."""
    b = np.asarray(bits, np.int64).reshape(-1)
    tg = np.zeros((b.size, l, k + 1, k + 1, N), np.int64)
    for p in range(l):
        for j in range(k + 1):
            tg[:, p, j, j, 0] = b << (32 - (p + 1) * beta)
    return wrap32(tg).astype(np.int32)


def mk_trivial_uni(bits, N, l, beta):
    """RGSW.UniEnc (mk_internals.jl:185-227) of each bit by a party whose key material is zero (s = 0, r = 0, no noise, c1 = f1 = 0):
    (c0, c1, d0, d1, f0, f1), int32 [S][l][N] each, c0 and d1 holding b g_p on the constant term."""
    b = np.asarray(bits, np.int64).reshape(-1)
    mg = np.zeros((b.size, l, N), np.int64)
    for p in range(l):
        mg[:, p, 0] = b << (32 - (p + 1) * beta)
    mg = wrap32(mg).astype(np.int32)
    zero = np.zeros_like(mg)
    return mg, zero, zero, mg.copy(), zero, zero


def mk_trivial_selectors(bits, owners, N, l, beta, P):
    """The expansion (RGSW.Expand, mk_internals.jl:304-345, against public keys that are zero) of mk_trivial_uni in the layout
    x[l][P] | y[l][P] | c0[l] | c1[l] (:243-271): int32 [S][2 l P + 2 l][N] with y[p][owner] = c0[p] = b g_p on coefficient 0, else 0."""
    mg = mk_trivial_uni(bits, N, l, beta)[0]
    who = np.asarray(owners).reshape(-1)
    out = np.zeros((mg.shape[0], 2 * l * P + 2 * l, N), np.int32)
    for s in range(mg.shape[0]):
        for p in range(l):
            out[s, l * P + p * P + int(who[s])] = mg[s, p]
        out[s, 2 * l * P:2 * l * P + l] = mg[s]
    return out


def extract0(sample):
    """tlwe_extract_sample / mk_tlwe_extract_sample at coefficient 0 on plain words [polys][N] -> int32 [(polys - 1) N + 1]: each mask
    polynomial as p[0], -p[N-1], ..., -p[1] (polynomials.jl:32-35), then body[0].  Written out here so that the known answer stays
    free of the schoolbook classes."""
    s = np.asarray(sample, np.int64)
    masks = [np.concatenate([p[:1], -p[:0:-1]]) for p in s[:-1]]
    return wrap32(np.concatenate(masks + [s[-1][:1]])).astype(np.int32)


def known_tree(table, bits):
    """table[address] with address = sum_v bits[v] 2^v: what a CMUX tree over trivial selectors returns on multiples of h."""
    return np.asarray(table)[sum(int(b) << v for v, b in enumerate(bits))]


def known_net(net, table, bits):
    """CmuxNet.evaluate_clear on whole samples: int32 [F][polys][N]."""
    return np.stack(net.evaluate_clear([np.asarray(t) for t in table], [int(b) for b in bits])).astype(np.int32)


def known_rot_net(net, table, bits):
    """RotNet.evaluate_clear polynomial by polynomial (it takes plain polynomials [N]), wrapped to 32-bit words: int32 [F][polys][N]."""
    t = np.asarray(table, np.int64)
    polys = [np.stack(net.evaluate_clear(list(t[:, c]), [int(b) for b in bits])) for c in range(t.shape[1])]      # [polys][F][N]
    return wrap32(np.stack(polys, axis=1)).astype(np.int32)
