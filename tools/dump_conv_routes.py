#!/usr/bin/env python
"""Dump the conv routing answers of a built libmi355x_kernels.so as one JSON document.

    python tools/dump_conv_routes.py path/to/libmi355x_kernels.so [--out FILE] [--new]

Pure host arithmetic: no GPU needed (without one the panel plan's CU count falls back to 256, the
MI355X's).  Only plain ctypes and only the query / setter symbols every revision of the library
has, so the same tool records an older build's answers (tests/data/conv_routes_parent.json, which
tests/test_conv_route_cpu.py holds the current code to).  --new adds what needs the current
library: mi_dgrad_stat_rows_g, also on 3x3 pad-0 shapes, and every row count again with the panel
and 256-wide conv routes switched off ("nt_only").  Run it with no MI355X_DP_* variable set.
"""
import argparse
import ctypes
import json
import sys

INT_MAX = 2**31 - 1

# setter -> default (what an environment without MI355X_DP_* variables gives)
DEFAULTS = {
    "mi_set_panel": 1,
    "mi_set_conv256_min_tiles": 96,
    "mi_set_conv256_min_k": 512,
    "mi_set_panel_first": 0,
    "mi_set_g256_bm224": 1,
}
SETTINGS = [
    ("default", []),
    ("panel0", [("mi_set_panel", 0)]),
    ("panel2", [("mi_set_panel", 2)]),
    ("panel5", [("mi_set_panel", 5)]),
    ("panel6", [("mi_set_panel", 6)]),
    ("conv256_forced", [("mi_set_conv256_min_tiles", 1), ("mi_set_conv256_min_k", 0)]),
    ("panel_first", [("mi_set_panel_first", 1)]),
    ("bm224_off", [("mi_set_g256_bm224", 0)]),
]
# the queries recorded per (setting, shape), in this order
QUERIES = ["conv_stat_rows_g", "dgrad_stat_rows", "conv_stat_rows", "conv_nol_ok", "conv_fbb_route", "conv_fbb_rows",
           "panel_rows_fwd", "panel_rows_dgrad", "g256_rows_fwd", "g256_rows_dgrad"]


def _out(h, r, stride, pad):
    return (h + 2 * pad - r) // stride + 1


def resnet_convs(depth, batch, size):
    """(Nb, H, W, C, K, R, S, stride, pad) of every conv of a torchvision-layout ResNet (stride on the
    3x3), the stem on its 8-channel padded input"""
    blocks = {18: (2, 2, 2, 2), 50: (3, 4, 6, 3), 152: (3, 8, 36, 3)}[depth]
    exp = 1 if depth == 18 else 4
    convs = [(batch, size, size, 8, 64, 7, 7, 2, 3)]
    h = _out(_out(size, 7, 2, 3), 3, 2, 1)  # stem, max pool
    inpl = 64
    for li, n in enumerate(blocks):
        planes = 64 << li
        for b in range(n):
            s = 2 if (li > 0 and b == 0) else 1
            ho = _out(h, 3, s, 1)
            if exp == 1:
                convs += [(batch, h, h, inpl, planes, 3, 3, s, 1), (batch, ho, ho, planes, planes, 3, 3, 1, 1)]
            else:
                convs += [(batch, h, h, inpl, planes, 1, 1, 1, 0), (batch, h, h, planes, planes, 3, 3, s, 1),
                          (batch, ho, ho, planes, planes * 4, 1, 1, 1, 0)]
            if s != 1 or inpl != planes * exp:
                convs.append((batch, h, h, inpl, planes * exp, 1, 1, s, 0))
            inpl, h = planes * exp, ho
    return convs


EDGE_SHAPES = [
    # 3x3 pad 1 and 1x1 with C = K = 64 / 64 -> 256 around M = 16384 (PN_MIN_M)
    (63, 16, 16, 64, 64, 3, 3, 1, 1), (64, 16, 16, 64, 64, 3, 3, 1, 1), (65, 16, 16, 64, 64, 3, 3, 1, 1),
    (63, 16, 16, 64, 256, 1, 1, 1, 0), (64, 16, 16, 64, 256, 1, 1, 1, 0), (65, 16, 16, 64, 256, 1, 1, 1, 0),
    # 1x1 stride 2; 5x5 pad 2; the C = 8 stem and a C = 8 conv that is not the stem
    (8, 28, 28, 256, 512, 1, 1, 2, 0), (8, 27, 27, 64, 128, 1, 1, 2, 0), (8, 28, 28, 64, 64, 5, 5, 1, 2),
    (2, 64, 64, 8, 64, 7, 7, 2, 3), (2, 32, 32, 8, 64, 3, 3, 1, 1),
    # K = 72 (no multiple of 64)
    (4, 14, 14, 64, 72, 3, 3, 1, 1), (4, 14, 14, 64, 72, 1, 1, 1, 0),
    # cdiv(M,128) * cdiv(N,128) = 508 | 512 (nt_choice border), 1x1 and 3x3
    (127, 16, 16, 64, 256, 1, 1, 1, 0), (128, 16, 16, 64, 256, 1, 1, 1, 0),
    (127, 16, 16, 64, 256, 3, 3, 1, 1), (128, 16, 16, 64, 256, 3, 3, 1, 1),
    # N = 64 against N = 128
    (32, 16, 16, 64, 64, 3, 3, 1, 1), (32, 16, 16, 64, 128, 3, 3, 1, 1),
    (32, 16, 16, 128, 64, 1, 1, 1, 0), (32, 16, 16, 128, 128, 1, 1, 1, 0),
    # cdiv(M,256) * cdiv(N,256) = 94 | 96 with R*S*C = 576 >= 512
    (47, 16, 16, 64, 512, 3, 3, 1, 1), (48, 16, 16, 64, 512, 3, 3, 1, 1),
    # 1x1 with K = 1024, C = 256 and its transpose (32-column panels at depth 1024)
    (32, 14, 14, 256, 1024, 1, 1, 1, 0), (128, 14, 14, 256, 1024, 1, 1, 1, 0),
    (32, 14, 14, 1024, 256, 1, 1, 1, 0), (128, 14, 14, 1024, 256, 1, 1, 1, 0),
]
# 3x3 pad 0 / stride 1 (--new only: the old data-gradient query has no pad argument)
PAD0_SHAPES = [(2, 14, 14, 64, 64, 3, 3, 1, 0), (64, 18, 18, 64, 64, 3, 3, 1, 0), (32, 30, 30, 128, 128, 3, 3, 1, 0),
               (256, 58, 58, 64, 64, 3, 3, 1, 0)]


def all_shapes():
    seen, out = set(), []
    for batch, size in ((256, 224), (32, 32), (2, 64)):
        for depth in (18, 50, 152):
            for c in resnet_convs(depth, batch, size):
                if c not in seen:
                    seen.add(c)
                    out.append(c)
    for c in EDGE_SHAPES:
        if c not in seen:
            seen.add(c)
            out.append(c)
    return [list(c) + [_out(c[1], c[5], c[7], c[8]), _out(c[2], c[6], c[7], c[8])] for c in out]


def answers(lib, shape):
    Nb, H, W, C, K, R, S, s, p, P, Q = shape
    Mf, Md = Nb * P * Q, Nb * H * W
    return [
        lib.mi_conv_stat_rows_g(Nb, H, W, C, K, R, S, s, p, P, Q),
        lib.mi_dgrad_stat_rows(Nb, H, W, C, P, Q, s, K, R * S),
        lib.mi_conv_stat_rows(Mf, K, C, R * S),
        lib.mi_conv_nol_ok(Nb, H, W, C, K, R, S, s, p, P, Q),
        lib.mi_conv_fbb_route(Md, C, K),
        lib.mi_conv_fbb_rows(Md, C, K),
        lib.mi_panel_stat_rows2(Mf, K, R * S * C, 0),
        lib.mi_panel_stat_rows2(Md, C, R * S * K, 1),
        lib.mi_g256_stat_rows(Mf, K, R * S * C),
        lib.mi_g256_stat_rows(Md, C, R * S * K),
    ]


def apply(lib, calls):
    for name, value in list(DEFAULTS.items()) + list(calls):
        getattr(lib, name)(value)


def dump(lib_path, new=False):
    lib = ctypes.CDLL(lib_path)
    shapes = all_shapes()
    doc = {"shape_fields": ["Nb", "H", "W", "C", "K", "R", "S", "stride", "pad", "P", "Q"], "shapes": shapes,
           "settings": [{"name": n, "calls": [list(c) for c in calls]} for n, calls in SETTINGS],
           "queries": QUERIES, "answers": {}}
    for name, calls in SETTINGS:
        apply(lib, calls)
        doc["answers"][name] = [answers(lib, sh) for sh in shapes]
    if new:
        pad0 = [list(c) + [_out(c[1], 3, 1, 0), _out(c[2], 3, 1, 0)] for c in PAD0_SHAPES]
        doc["new"] = {"pad0_shapes": pad0, "dgrad_stat_rows_g": {}, "pad0_dgrad_stat_rows_g": {}, "nt_only": {}}

        def dg(sh):
            Nb, H, W, C, K, R, S, s, p, P, Q = sh
            return lib.mi_dgrad_stat_rows_g(Nb, H, W, C, K, R, S, s, p, P, Q)

        for name, calls in SETTINGS:
            apply(lib, calls)
            doc["new"]["dgrad_stat_rows_g"][name] = [dg(sh) for sh in shapes]
            doc["new"]["pad0_dgrad_stat_rows_g"][name] = [dg(sh) for sh in pad0]
            # the same setting without the panel and 256-wide conv routes: [forward rows, dgrad rows]
            apply(lib, list(calls) + [("mi_set_panel", 0), ("mi_set_conv256_min_tiles", INT_MAX)])
            doc["new"]["nt_only"][name] = [[answers(lib, sh)[0], dg(sh)] for sh in shapes]
    apply(lib, [])
    return doc


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("lib")
    ap.add_argument("--out")
    ap.add_argument("--new", action="store_true")
    a = ap.parse_args(argv)
    text = json.dumps(dump(a.lib, a.new), separators=(",", ":")).replace("]],", "]],\n")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    else:
        sys.stdout.write(text + "\n")


if __name__ == "__main__":
    main()
