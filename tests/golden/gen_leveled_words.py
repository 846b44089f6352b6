#!/usr/bin/env python3
"""Writes tests/golden/leveled_words.json: the output words of the seven leveled calls as a build of the library computes them, for
tests/test_leveled_words.py to hold later builds to.  The existing tests compare the level kernels with integer schoolbooks where a
parameter set is exact and with each other where it is not; this file pins the words themselves, also where rounding is inexact, so the
kernels cannot drift together.

    python tests/golden/gen_leveled_words.py          (on a GPU, with the library of the commit that is the yardstick)

Only the public Python API is used, so the script runs unchanged on an older checkout.  Per case: the SHA-256 of the output array
(int32, C order), its first 8 words and tfhe_last_kernel_name.  Selectors and samples are arbitrary 32-bit words of a seeded generator
(the kernels accept any); the keys come from the same generator, and out_form 2 reads the keyswitch key.

Cases, for (N, k, l, beta) = (64, 1, 3, 8) and (1024, 2, 2, 10), multi-key (N, P, l, beta) = (64, 2, 3, 8) and (1024, 2, 2, 10) (a
multi-key sample has k = 1), B = 3 rows, tables [1, 0, 1], every out_form, accumulators in LDS and in global memory (option anyn_spec):
  extern_mul, cmux_tree of depth 2, a 2-level cmux_net with a copy node and a shared source, a 2-level rot_net with a rotated copy, a
  rotation >= N and a node with rot0 != rot1 on one source, mk_extern_mul, mk_cmux_tree of depth 2 with selectors of both parties, and
  the same cmux_net as mk_cmux_net."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "leveled_words.json")
SETS = {"single_key": [(64, 1, 3, 8), (1024, 2, 2, 10)],       # N, k, l, beta
        "multi_key": [(64, 2, 3, 8), (1024, 2, 2, 10)]}        # N, P, l, beta
B, T, S, LWE_N = 3, 2, 4, 6
INDEX = np.array([1, 0, 1], np.int32)
TREE_SEL = np.array([[0, 1], [3, 2], [1, 1]], np.int32)                    # [B][depth 2]; multi-key: selectors 0, 3 are party 0's, 1, 2 party 1's
NET_SEL = np.array([[0, 1, 2], [3, 2, 0], [1, 1, 3]], np.int32)            # [B][V 3]
PARTY_OF = np.array([0, 1, 1, 0], np.int32)
NET_WIDTHS = [3, 2]
NET_NODES = [[0, 1, 0], [2, 2, 1], [1, 3, 2],                              # level 0 over E = 4 entries: entry 1 feeds two nodes, node 1 copies
             [0, 1, 1], [1, 2, 0]]                                         # level 1: the copy feeds both nodes


def rot_nodes(N):
    return [[0, 1, 0, 5, N + 3], [2, 2, 1, 7, 7], [1, 1, 2, 0, 2 * N - 1],     # a rotation >= N; a rotated copy; one source, rot0 != rot1
            [0, 1, 1, 0, 0], [1, 2, 0, N, 1]]


def _words(rng, *shape):
    return rng.integers(-2**31, 2**31, size=shape, dtype=np.int64).astype(np.int32)


def _record(eng, out):
    out = np.ascontiguousarray(out, dtype=np.int32)
    return {"sha256": hashlib.sha256(out.tobytes()).hexdigest(), "first": [int(v) for v in out.reshape(-1)[:8]], "kernel": eng.last_kernel_name()}


def _both_placements(eng, calls):
    got = {}
    for spec in (-1, 1):
        eng.set_option("anyn_spec", spec)
        for name, call in calls:
            got[f"{name},spec={spec}"] = _record(eng, call())
    eng.set_option("anyn_spec", -1)
    return got


def single_key(tfhe, N, k, l, beta):
    """{case: record} of the four single-key calls at one parameter set."""
    from tfhe_jl_amd import leveled
    rng = np.random.default_rng(9100 + N + k)
    sk, ck = tfhe.make_key_pair(rng, tfhe.SchemeParameters(LWE_N, 1 / 2**15, N, k, l, beta, 9e-9, 8, 2, 1 / 2**15, 1))
    eng = ck.engine(0)
    eng.tgsw_load(_words(rng, S, l, k + 1, k + 1, N))
    data = _words(rng, T, 4, k + 1, N)
    net = leveled.CmuxNet(NET_WIDTHS, NET_NODES, entries=4, variables=3)
    rot = leveled.RotNet(NET_WIDTHS, rot_nodes(N), N, entries=4, variables=3)
    calls = [("extern_mul", lambda: eng.extern_mul(data[0, :B], NET_SEL[:, 0]))]
    for form in (0, 1, 2):
        calls += [(f"cmux_tree,form={form}", lambda form=form: eng.cmux_tree(data, TREE_SEL, table_index=INDEX, out_form=form)),
                  (f"cmux_net,form={form}", lambda form=form: eng.cmux_net(data, net, NET_SEL, table_index=INDEX, out_form=form)),
                  (f"rot_net,form={form}", lambda form=form: eng.rot_net(data, rot, NET_SEL, table_index=INDEX, out_form=form))]
    got = _both_placements(eng, calls)
    ck.close()
    return got


def multi_key(tfhe, N, P, l, beta):
    """{case: record} of the three multi-key calls at one parameter set of P parties."""
    from tfhe_jl_amd import leveled
    rng = np.random.default_rng(9200 + N + P)
    p = tfhe.SchemeParameters(4, 0.012467, N, 1, l, beta, 3.29e-10, 8, 2, 2.44e-5, P)
    shared = tfhe.SharedKey(rng, p)
    ck = tfhe.MKCloudKey([tfhe.CloudKeyPart(rng, tfhe.SecretKey(rng, p), shared) for _ in range(P)])
    eng = ck.engine(0)
    eng.mk_tgsw_load(_words(rng, S, 2 * l * P + 2 * l, N), PARTY_OF)
    data = _words(rng, T, 4, P + 1, N)
    net = leveled.CmuxNet(NET_WIDTHS, NET_NODES, entries=4, variables=3)
    calls = [("mk_extern_mul", lambda: eng.mk_extern_mul(data[0, :B], NET_SEL[:, 0]))]
    for form in (0, 1, 2):
        calls += [(f"mk_cmux_tree,form={form}", lambda form=form: eng.mk_cmux_tree(data, TREE_SEL, table_index=INDEX, out_form=form)),
                  (f"mk_cmux_net,form={form}", lambda form=form: eng.mk_cmux_net(data, net, NET_SEL, table_index=INDEX, out_form=form))]
    got = _both_placements(eng, calls)
    ck.close()
    return got


FAMILIES = {"single_key": single_key, "multi_key": multi_key}


def key(family, N, kp, l, beta):
    return f"{family},N={N},{'k' if family == 'single_key' else 'P'}={kp},l={l},beta={beta}"


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import tfhe_jl_amd as tfhe
    golden = {key(f, *s): fn(tfhe, *s) for f, fn in FAMILIES.items() for s in SETS[f]}
    json.dump(golden, open(sys.argv[1] if len(sys.argv) > 1 else OUT, "w"), indent=0, sort_keys=True)
    print(sum(len(v) for v in golden.values()), "cases")
