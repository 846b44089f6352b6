#!/usr/bin/env python3
"""Writes tests/golden/rotation_words.json: what the four TLWE rotation calls (tfhe_blind_rotate_batch, tfhe_mk_blind_rotate_batch,
tfhe_blind_rotate_level, tfhe_mk_blind_rotate_level), the two level network calls (tfhe_rot_net_level, tfhe_mk_rot_net_level) and the
(MK) TLWE table compute and refuse as a build of the library does it, for tests/test_rotation_words.py to hold later builds to.  The
other tests compare the level calls with the batch calls; this file pins the words, the kernel names, the return codes and the messages
themselves, so the two families cannot drift together.

    python tests/golden/gen_rotation_words.py          (on a GPU, with the library of the commit that is the yardstick)

Only the public Python API is used, and raw `_lib` calls for the refusals, so the script runs unchanged on an older checkout.  Per
successful case: the SHA-256 of the int32 output, its first 8 words and tfhe_last_kernel_name; after a level call the output is the
written slots or wires, and the whole TLWE table and the whole wire table are hashed too.  Per refusal: [rc, message].  Keys,
selectors, samples and wires are arbitrary 32-bit words of a seeded generator (the kernels accept any).

Sets: single-key (N, k, l, beta) = (64, 1, 3, 8) and (1024, 2, 2, 10) with LWE n = 6; multi-key (N, P, l, beta) = (64, 2, 3, 8) and
(32, 3, 2, 8) with n = 4.  B = 3 rows, T = 2 accumulators, 16 slots, 48 wires, accumulators in LDS and in global memory (anyn_spec).
  batch rotation   in_form 0 / 1 x (out_form, n_out) = (0, 1), (1, 1), (1, 4), (2, 1), (2, 4) x (sel, acc_index) = (NULL, NULL) /
                   (a permutation, [1, 0, 1])
  level rotation   rows of 0, 1 and 2 terms x (out_form, n_out) = (0, 1), (2, 1), (2, 4) x cst NULL / given, sel NULL / a permutation;
                   a call without terms, cst given / NULL, and on the multi-key side also without a wire table
  level network    the two-level network of tests/test_tlwe_levels.py x out_form 0 / 2 x table_first NULL / [0, 2, 1]
  table            alloc, partial upload, downloads, re-alloc, alloc(0)
  refusals (first set of each kind)   the argument cases, the state sequences and the injected allocation failures of
                   tests/test_tlwe_levels.py and tests/test_mk_tlwe_levels.py"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "rotation_words.json")
SETS = {"single_key": [(64, 1, 3, 8), (1024, 2, 2, 10)],       # N, k, l, beta
        "multi_key": [(64, 2, 3, 8), (32, 3, 2, 8)]}           # N, P, l, beta
LWE_N = {"single_key": 6, "multi_key": 4}
B, T, SLOTS, WIRES = 3, 2, 16, 48
INDEX = np.array([1, 0, 1], np.int32)
ACC_SLOT, OUT_SLOT = [1, 1, 2], [8, 9, 10]
TERM_START, TERM_WIRE, TERM_COEF, CST = [0, 0, 1, 3], [4, 5, 4], [1, -2, 3], [5, 6, 7]
NET_FIRST = [0, 2, 1]


def _words(rng, *shape):
    return rng.integers(-2**31, 2**31, size=shape, dtype=np.int64).astype(np.int32)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.int32).tobytes()).hexdigest()


def _record(eng, out):
    out = np.ascontiguousarray(out, dtype=np.int32)
    return {"sha256": _sha(out), "first": [int(v) for v in out.reshape(-1)[:8]], "kernel": eng.last_kernel_name()}


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def two_level_net(leveled, N):
    nodes = [(0, 1, 0, 0, 1), (2, 2, 1, 5, 5), (3, 1, 1, N, 2 * N - 1), (0, 2, 2, 0, 0), (1, 1, 0, 0, 0)]
    return leveled.RotNet([3, 2], nodes, N, entries=4, variables=3)


class Kind:
    """One context of a family with its selectors loaded, and the family's names for the calls."""

    def __init__(self, tfhe, family, N, kp, l, beta):
        self.tfhe, self.mk, self.N, self.l = tfhe, family == "multi_key", N, l
        n = LWE_N[family]
        rng = self.rng = np.random.default_rng((9300 if self.mk else 9400) + N + kp)
        if self.mk:
            P = self.P = kp
            self.params = tfhe.SchemeParameters(n, 0.012467, N, 1, l, beta, 3.29e-10, 8, 2, 2.44e-5, P)
            shared = tfhe.SharedKey(rng, self.params)
            self.parts = [tfhe.CloudKeyPart(rng, tfhe.SecretKey(rng, self.params), shared) for _ in range(P)]
            self.ck = tfhe.MKCloudKey(self.parts)
            self.polys, self.steps, self.pre = P + 1, P * n, "mk_"
        else:
            self.params = tfhe.SchemeParameters(n, 1 / 2**15, N, kp, l, beta, 9e-9, 8, 2, 1 / 2**15, 1)
            sk, self.ck = tfhe.make_key_pair(rng, self.params)
            self.polys, self.steps, self.pre = kp + 1, n, ""
        self.S = self.steps + 2
        self.tgsw = _words(rng, self.S, 2 * l * self.P + 2 * l, N) if self.mk else _words(rng, self.S, l, kp + 1, kp + 1, N)
        self.party_of = (np.arange(self.S) % kp).astype(np.int32)
        self.full = _words(rng, SLOTS, self.polys, N)
        self.allw = _words(rng, WIRES, self.steps + 1)
        self.perm = rng.permutation(self.S)[:self.steps].astype(np.int32)
        self.eng = self.ck.engine(0)
        self.load_selectors(self.eng)

    def call(self, eng, name, *a, **kw):
        return getattr(eng, self.pre + name)(*a, **kw)

    def raw(self, name):
        return getattr(self.eng._lib, "tfhe_" + self.pre + name)

    def load_selectors(self, eng):
        if self.mk:
            eng.mk_tgsw_load(self.tgsw, self.party_of)
        else:
            eng.tgsw_load(self.tgsw)

    def load_bootstrap_key(self, eng):
        if self.mk:
            eng.mk_load_bootstrap_key(self.ck.bootstrap_key, self.P)
        else:
            eng.load_bootstrap_key(self.ck.bootstrap_key)

    def wires_alloc(self, eng, count):
        (eng.mk_wires_alloc if self.mk else eng.wires_alloc)(count)

    def tables(self, eng, wires=True):
        self.call(eng, "tlwe_alloc", SLOTS)
        self.call(eng, "tlwe_upload", 0, self.full)
        if wires:
            self.wires_alloc(eng, WIRES)
            eng.wires_upload(0, self.allw)

    def level_record(self, out, wires=True):
        """The record of a level call: `out` (the written slots or wires), the whole tables; then the tables as they were."""
        eng = self.eng
        rec = _record(eng, out)
        rec["table"] = _sha(self.call(eng, "tlwe_download", 0, SLOTS))
        self.call(eng, "tlwe_upload", 0, self.full)
        if wires:
            rec["wires"] = _sha(eng.wires_download(0, WIRES))
            eng.wires_upload(0, self.allw)
        return rec


def batch_cases(K):
    eng, rng = K.eng, K.rng
    acc = _words(rng, T, K.polys, K.N)
    rows = {0: _words(rng, B, K.steps + 1), 1: rng.integers(0, 2 * K.N, (B, K.steps + 1)).astype(np.int32)}
    got = {}
    for in_form in (0, 1):
        for out_form, n_out in ((0, 1), (1, 1), (1, 4), (2, 1), (2, 4)):
            for tag, sel, idx in (("plain", None, None), ("mapped", K.perm, INDEX)):
                out = K.call(eng, "blind_rotate", acc, rows[in_form], sel=sel, acc_index=idx, in_form=in_form, n_out=n_out, out_form=out_form)
                got[f"batch,in={in_form},form={out_form},n_out={n_out},{tag}"] = _record(eng, out)
    return got


def level_cases(K):
    eng = K.eng
    got = {}

    def rotate(name, start, cst, sel, out_form, n_out, wires=True):
        out_wires = [20 + 2 * i for i in range(B * n_out)]
        K.call(eng, "blind_rotate_level", ACC_SLOT, start, TERM_WIRE if start[-1] else [], TERM_COEF if start[-1] else [], cst=cst, sel=sel, n_out=n_out,
               out_form=out_form, out_slot=OUT_SLOT if out_form == 0 else None, out_wires=out_wires if out_form == 2 else None)
        out = K.call(eng, "tlwe_download", 0, SLOTS)[OUT_SLOT] if out_form == 0 else eng.wires_gather(out_wires)
        got[name] = K.level_record(out, wires)

    for out_form, n_out in ((0, 1), (2, 1), (2, 4)):
        for tag, cst, sel in (("plain", None, None), ("cst,sel", CST, K.perm)):
            rotate(f"level,form={out_form},n_out={n_out},{tag}", TERM_START, cst, sel, out_form, n_out)
        rotate(f"level,form={out_form},n_out={n_out},no terms", [0, 0, 0, 0], CST, None, out_form, n_out)
    rotate("level,form=0,n_out=1,no terms,no cst", [0, 0, 0, 0], None, K.perm, 0, 1)
    return got


def level_cases_without_wires(K):
    """(the multi-key call without terms stages its rows on the host: it must not ask the wire table for their width)"""
    eng = K.eng
    eng.wires_alloc(0)
    got = {}
    for tag, cst in (("cst", CST), ("no cst", None)):
        K.call(eng, "blind_rotate_level", ACC_SLOT, [0, 0, 0, 0], [], [], cst=cst, out_form=0, out_slot=OUT_SLOT)
        got[f"level,no wire table,{tag}"] = K.level_record(K.call(eng, "tlwe_download", 0, SLOTS)[OUT_SLOT], wires=False)
    K.wires_alloc(eng, WIRES)
    eng.wires_upload(0, K.allw)
    return got


def net_cases(K):
    from tfhe_jl_amd import leveled
    eng = K.eng
    net = two_level_net(leveled, K.N)
    sel = K.rng.integers(0, K.S, (B, 3)).astype(np.int32)
    out_wires = [13, 40, 21, 12, 47, 30]
    got = {}
    for out_form in (0, 2):
        for tag, first in (("absolute", None), ("first", NET_FIRST)):
            K.call(eng, "rot_net_level", net, sel, table_first=first, out_form=out_form, out_first=8, out_wires=out_wires if out_form == 2 else None)
            out = K.call(eng, "tlwe_download", 8, 6) if out_form == 0 else eng.wires_gather(out_wires)
            got[f"net,form={out_form},{tag}"] = K.level_record(out)
    return got


def table_cases(K):
    """(the table is freed and made again: as it was afterwards)"""
    eng, got = K.eng, {}
    part = _words(K.rng, 3, K.polys, K.N)
    K.call(eng, "tlwe_upload", 5, part)
    got["table,partial"] = _record(eng, K.call(eng, "tlwe_download", 4, 5))
    got["table,whole"] = _record(eng, K.call(eng, "tlwe_download", 0, SLOTS))
    got["table,empty range"] = _record(eng, K.call(eng, "tlwe_download", SLOTS, 0))
    K.call(eng, "tlwe_alloc", 4)
    K.call(eng, "tlwe_upload", 1, part)
    got["table,realloc"] = _record(eng, K.call(eng, "tlwe_download", 1, 3))
    K.call(eng, "tlwe_alloc", 0)
    one = np.zeros((1, K.polys, K.N), np.int32)
    lib, h = eng._lib, eng._h
    for name, call in (("download", lambda: K.raw("tlwe_download")(h, 0, 1, _ptr(one))), ("upload", lambda: K.raw("tlwe_upload")(h, 0, 1, _ptr(one))),
                       ("alloc -1", lambda: K.raw("tlwe_alloc")(h, -1)), ("alloc 2^31", lambda: K.raw("tlwe_alloc")(h, 2**31))):
        got[f"table,freed,{name}"] = [call(), lib.tfhe_last_error(h).decode()]
    K.tables(eng, wires=False)
    for name, first, count in (("before", -1, 1), ("past", SLOTS, 1), ("across the end", SLOTS - 1, 2), ("negative", 0, -1), ("NULL", 0, 1)):
        buf = None if name == "NULL" else _ptr(np.zeros((2, K.polys, K.N), np.int32))
        for way in ("upload", "download"):
            got[f"table,{way},{name}"] = [K.raw("tlwe_" + way)(h, first, count, buf), lib.tfhe_last_error(h).decode()]
    return got


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
ROT_OK = dict(acc_slot=ACC_SLOT, term_start=TERM_START, term_wire=TERM_WIRE, term_coef=TERM_COEF, cst=CST, sel=None, n_out=1, out_form=0, out_slot=OUT_SLOT,
              out_wires=None, B=3)
ROT_CASES = [dict(out_slot=[8, 9, 9]), dict(out_slot=[8, 9, 2]), dict(out_slot=[8, 9, SLOTS]), dict(out_slot=[-1, 9, 10]), dict(acc_slot=[1, SLOTS, 2]),
             dict(acc_slot=[1, -1, 2]), dict(term_wire=[4, WIRES, 4]), dict(term_wire=[4, -1, 4]), dict(term_start=[1, 1, 1, 3]), dict(term_start=[0, 2, 1, 3]),
             dict(n_out=2), dict(n_out=0), dict(out_form=1), dict(out_form=3), dict(out_form=-1),
             dict(out_form=2, out_wires=[20, 21, 21]), dict(out_form=2, out_wires=[20, 21, 5]), dict(out_form=2, out_wires=[20, 21, WIRES]),
             dict(out_form=2, n_out=32, out_wires=list(range(12, 12 + 96))), dict(out_form=2, n_out=3, out_wires=list(range(12, 21))),
             dict(B=-1), dict(acc_slot=None), dict(term_start=None), dict(out_slot=None), dict(out_form=2), dict(term_wire=None), dict(term_coef=None), dict(B=0),
             dict(out_form=2, n_out=64, out_wires=[20])]
NET_OK = dict(table_first=NET_FIRST, E=4, V=3, out_form=0, out_first=8, out_wires=None, B=3)
WIRES6 = dict(out_form=2, out_wires=[20, 21, 22, 23, 24, 25])
NET_CASES = [dict(out_first=5), dict(out_first=11), dict(out_first=-1), dict(table_first=[0, 13, 1]), dict(table_first=[0, -1, 1]), dict(out_form=1), dict(out_form=3),
             dict(table_first=None, out_first=3), dict(out_form=2, out_wires=[20, 21, 22, 23, 24, 20]), dict(out_form=2, out_wires=[20, 21, 22, 23, 24, WIRES]),
             dict(out_form=2, out_wires=[20, 21, 22, 23, 24, -1]),
             dict(B=-1), dict(widths=None), dict(nodes=None), dict(sel=None), dict(E=0), dict(E=SLOTS + 1), dict(V=0), dict(levels=0), dict(out_form=2), dict(B=0)]


def _rot(K, eng, **over):
    a = dict(ROT_OK, **over)
    arr = {key: None if a[key] is None else np.asarray(a[key], np.int32) for key in ("acc_slot", "term_start", "term_wire", "term_coef", "cst", "sel", "out_slot", "out_wires")}
    rc = K.raw("blind_rotate_level")(eng._h, _ptr(arr["acc_slot"]), _ptr(arr["term_start"]), _ptr(arr["term_wire"]), _ptr(arr["term_coef"]), _ptr(arr["cst"]),
                                     _ptr(arr["sel"]), a["n_out"], a["out_form"], _ptr(arr["out_slot"]), _ptr(arr["out_wires"]), a["B"])
    return [rc, eng._lib.tfhe_last_error(eng._h).decode() if rc else ""]


def _net(K, eng, net, rows_sel, /, **over):
    a = dict(NET_OK, widths=net.widths, levels=net.levels, nodes=net.nodes, sel=rows_sel)
    a.update(over)
    arr = {key: None if a[key] is None else np.ascontiguousarray(a[key], np.int32) for key in ("table_first", "widths", "nodes", "sel", "out_wires")}
    rc = K.raw("rot_net_level")(eng._h, _ptr(arr["table_first"]), a["E"], _ptr(arr["widths"]), a["levels"], _ptr(arr["nodes"]), _ptr(arr["sel"]), a["V"],
                                a["out_form"], a["out_first"], _ptr(arr["out_wires"]), a["B"])
    return [rc, eng._lib.tfhe_last_error(eng._h).decode() if rc else ""]


def _batch(K, eng, acc, rows, **over):
    a = dict(T=T, acc_index=INDEX, steps=K.steps, in_form=0, sel=None, n_out=1, B=B, out_form=0)
    a.update(over)
    out = np.zeros(B * 32 * (K.polys * K.N + 1), np.int32)
    sel, idx = (None if a[key] is None else np.asarray(a[key], np.int32) for key in ("sel", "acc_index"))
    rc = K.raw("blind_rotate_batch")(eng._h, _ptr(acc), a["T"], _ptr(idx), _ptr(rows), a["steps"], a["in_form"], _ptr(sel), a["n_out"], _ptr(out), a["B"], a["out_form"])
    return [rc, eng._lib.tfhe_last_error(eng._h).decode() if rc else ""]


def refusal_cases(K):
    """The argument cases on the working context, then the state sequences on fresh ones, in the tests' order.  (Last on its context:
    after an injected allocation failure tfhe_last_error goes on reporting that failure to this thread.)"""
    from tfhe_jl_amd import leveled
    tfhe, eng, S = K.tfhe, K.eng, K.S
    net = two_level_net(leveled, K.N)
    sel = K.rng.integers(0, S, (3, 3)).astype(np.int32)
    got = {}

    def both(tag, e, rot_over, net_over):
        got[f"refuse,{tag},rot"] = _rot(K, e, **rot_over)
        got[f"refuse,{tag},net"] = _net(K, e, net, sel, **net_over)

    for over in ROT_CASES:
        got[f"refuse,rot,{over}"] = _rot(K, eng, **over)
    good = list(range(K.steps))
    got["refuse,rot,sel past"] = _rot(K, eng, sel=good[:-1] + [S])
    got["refuse,rot,sel negative"] = _rot(K, eng, sel=good[:-1] + [-1])
    for over in NET_CASES:
        got[f"refuse,net,{over}"] = _net(K, eng, net, sel, **over)
    bad_nodes = net.nodes.copy(); bad_nodes[3, 1] = 3
    bad_sel = sel.copy(); bad_sel[1, 1] = S
    got["refuse,net,bad nodes"] = _net(K, eng, net, sel, nodes=bad_nodes)
    got["refuse,net,bad sel"] = _net(K, eng, net, sel, sel=bad_sel)
    # the batch calls
    acc, rows = _words(K.rng, T, K.polys, K.N), _words(K.rng, B, K.steps + 1)
    for over in (dict(B=-1), dict(steps=0), dict(steps=65537), dict(in_form=2), dict(out_form=3), dict(T=0), dict(T=2**31), dict(n_out=3), dict(n_out=64),
                 dict(n_out=2), dict(out_form=1, n_out=16, B=2**28), dict(sel=good[:-1] + [S]), dict(steps=S + 1), dict(acc_index=[0, T, 0]), dict(in_form=1), dict(B=0)):
        got[f"refuse,batch,{over}"] = _batch(K, eng, acc, rows, **over)
    # the state a level call needs, refused before the arguments are looked at
    eng.set_option("measure_margin", 1)
    both("measure_margin", eng, dict(out_slot=[8, 9, 9]), dict(out_first=5))
    got["refuse,measure_margin,batch"] = _batch(K, eng, acc, rows)
    eng.set_option("measure_margin", 0)
    raw = tfhe.Engine(K.params)
    if K.mk:
        got["refuse,no key,alloc"] = [K.raw("tlwe_alloc")(raw._h, 4), raw._lib.tfhe_last_error(raw._h).decode()]
        both("no key", raw, {}, {})
    K.load_bootstrap_key(raw)
    both("no table", raw, {}, {})
    K.call(raw, "tlwe_alloc", SLOTS)
    K.call(raw, "tlwe_upload", 0, K.full)
    both("no wire table", raw, {}, WIRES6)
    if K.mk:
        raw.wires_alloc(WIRES)                                               # a wire table with single-key rows
        both("single-key wires", raw, {}, WIRES6)
        raw.wires_alloc(0)
    both("no terms, arguments next", raw, dict(term_start=[0, 0, 0, 0], out_slot=[8, 9, 9]), dict(out_first=5))
    both("no selectors", raw, dict(term_start=[0, 0, 0, 0]), {})
    got["refuse,no selectors,batch"] = _batch(K, raw, acc, rows)
    K.load_selectors(raw)
    K.wires_alloc(raw, WIRES)
    raw.wires_upload(0, K.allw)
    both("no keyswitch key", raw, dict(out_form=2, out_wires=[20, 21, 22]), WIRES6)
    both("no keyswitch key, arguments first", raw, dict(out_form=2, out_wires=[20, 20, 20]), dict(out_form=2, out_wires=[20] * 6))
    got["refuse,no keyswitch key,batch"] = _batch(K, raw, acc, rows, out_form=2)
    both("runs without the keyswitch key", raw, {}, {})
    got["refuse,runs without the keyswitch key,table"] = _sha(K.call(raw, "tlwe_download", 0, SLOTS))
    raw.close()
    multi = K.ck.engine([0, 0])
    both("multi-device", multi, {}, {})
    got["refuse,multi-device,batch"] = _batch(K, multi, acc, rows)
    got["refuse,multi-device,alloc"] = [K.raw("tlwe_alloc")(multi._h, 4), multi._lib.tfhe_last_error(multi._h).decode()]
    # injected allocation failures at the first checkpoints of each call: where they sit, and what the call says
    lib = eng._lib
    for after in (1, 2, 3):
        for name, call in (("rot", lambda: _rot(K, eng)), ("rot wires", lambda: _rot(K, eng, out_form=2, out_wires=[20, 21, 22])), ("net", lambda: _net(K, eng, net, sel)),
                           ("net wires", lambda: _net(K, eng, net, sel, **WIRES6)), ("batch", lambda: _batch(K, eng, acc, rows))):
            assert lib.tfhe_set_option(None, b"debug_fail_alloc_after", after) == 0
            got[f"refuse,alloc failure {after},{name}"] = call()
            lib.tfhe_set_option(None, b"debug_fail_alloc_after", 0)
    K.call(eng, "tlwe_upload", 0, K.full)
    eng.wires_upload(0, K.allw)
    return got


def party_count_cases(K):
    """A table, a wire table and a keyswitch key for three parties under a bootstrapping key for two: refused in that order."""
    from tfhe_jl_amd import leveled
    tfhe, got = K.tfhe, {}
    net, sel = two_level_net(leveled, K.N), np.zeros((3, 3), np.int32)
    ck2 = tfhe.MKCloudKey(K.parts[:2])
    raw = tfhe.Engine(K.params)
    raw.mk_load_bootstrap_key(K.ck.bootstrap_key, 3)
    raw.mk_load_keyswitch_key(K.ck.keyswitch_key, 3)
    raw.mk_tlwe_alloc(SLOTS)
    raw.mk_wires_alloc(WIRES)
    raw.mk_load_bootstrap_key(ck2.bootstrap_key, 2)

    def both(tag, rot_over, net_over):
        got[f"refuse,{tag},rot"] = _rot(K, raw, **rot_over)
        got[f"refuse,{tag},net"] = _net(K, raw, net, sel, **net_over)

    both("3-party table", {}, {})
    raw.mk_tlwe_alloc(SLOTS)
    both("3-party wires", {}, WIRES6)
    raw.mk_wires_alloc(WIRES)
    both("3-party keyswitch key", dict(out_form=2, out_wires=[20, 21, 22]), WIRES6)
    both("2-party tables, no selectors", {}, {})
    raw.mk_tgsw_load(_words(K.rng, K.S, 2 * K.l * 2 + 2 * K.l, K.N), (np.arange(K.S) % 2).astype(np.int32))
    got["refuse,3-party keyswitch key,batch"] = _batch(K, raw, np.zeros(1, np.int32), np.zeros(1, np.int32), out_form=2)
    raw.close()
    ck2.close()
    return got


def other_kind_cases(tfhe, family, N, kp, l, beta):
    """Every entry point of the other family on a context of this one: refused by its kind."""
    K = Kind(tfhe, family, N, kp, l, beta)
    eng = K.eng
    lib, h = eng._lib, eng._h
    pre = "tfhe_" if K.mk else "tfhe_mk_"
    one, two = np.zeros(1, np.int32), np.zeros(2, np.int32)
    widths, nodes = np.ones(1, np.int32), np.zeros(5, np.int32)
    calls = {"alloc": lambda: getattr(lib, pre + "tlwe_alloc")(h, 4), "upload": lambda: getattr(lib, pre + "tlwe_upload")(h, 0, 0, None),
             "download": lambda: getattr(lib, pre + "tlwe_download")(h, 0, 0, None),
             "rot": lambda: getattr(lib, pre + "blind_rotate_level")(h, _ptr(one), _ptr(two), None, None, None, None, 1, 0, _ptr(one), None, 1),
             "net": lambda: getattr(lib, pre + "rot_net_level")(h, None, 1, _ptr(widths), 1, _ptr(nodes), _ptr(one), 1, 0, 1, None, 1),
             "batch": lambda: getattr(lib, pre + "blind_rotate_batch")(h, _ptr(one), 1, None, _ptr(two), 1, 0, None, 1, _ptr(one), 1, 0)}
    got = {f"refuse,other kind,{name}": [call(), lib.tfhe_last_error(h).decode()] for name, call in calls.items()}
    K.ck.close()
    return got


def cases(tfhe, family, N, kp, l, beta, refusals):
    """{case: record} of one parameter set; `refusals`: also the refusal sequences (the first set of each family)."""
    K = Kind(tfhe, family, N, kp, l, beta)
    K.tables(K.eng)
    got = {}
    for spec in (-1, 1):
        K.eng.set_option("anyn_spec", spec)
        for fn in (batch_cases, level_cases, net_cases) + ((level_cases_without_wires,) if K.mk else ()):
            got.update({f"{name},spec={spec}": rec for name, rec in fn(K).items()})
    K.eng.set_option("anyn_spec", -1)
    got.update(table_cases(K))
    if refusals:
        got.update(refusal_cases(K))
    if K.mk and K.P == 3:
        got.update(party_count_cases(K))
    K.ck.close()
    if refusals:
        got.update(other_kind_cases(tfhe, family, N, kp, l, beta))
    return got


def key(family, N, kp, l, beta):
    return f"{family},N={N},{'k' if family == 'single_key' else 'P'}={kp},l={l},beta={beta}"


ALL = [(f,) + s + (i == 0,) for f in sorted(SETS) for i, s in enumerate(SETS[f])]

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import tfhe_jl_amd as tfhe
    golden = {key(*a[:5]): cases(tfhe, *a) for a in ALL}
    json.dump(golden, open(sys.argv[1] if len(sys.argv) > 1 else OUT, "w"), indent=0, sort_keys=True)
    print(sum(len(v) for v in golden.values()), "cases")
