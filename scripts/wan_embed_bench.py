"""The Wan patch embedding on its own (fastgen_amd/csrc/wan_embed.hip) through its two op entry points, at the shapes the networks run:
    16 plain                   [1, 16, 21, 60, 104], D 1536  (Wan 2.1 1.3B; fg_op_wan_patch_embed, path 0: rows in registers)
    48 plain, 48 first frame   [1, 48, 21, 44, 80], D 3072   (Wan2.2 TI2V-5B; fg_op_wan_patch_embed, path 0: phased, path 1: per output)
    96                         [1, 96, 21, 60, 104], D 1536  (the VACE control video; fg_op_wan_vace_patch_embed, paths 0 and 1)
us per launch from device events, median / min / max of 10 launches after 3 warm-ups; one JSON line per case.  The concat view (Wan 2.1
I2V) has no op entry point: its kernel time comes from a kernel trace of `wan_bench.py --bidirectional --i2v --trace=CALLS`.
    python scripts/wan_embed_bench.py"""
import json

import torch

from fastgen_amd import _lib
from fastgen_amd.networks._engine import ptr

L = _lib.lib()


def timeit(fn, n=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


# (name, channels, frames, height, width, D, first frame, paths)
CASES = (("16 plain", 16, 21, 60, 104, 1536, False, (0,)),
         ("48 plain", 48, 21, 44, 80, 3072, False, (0, 1)),
         ("48 first frame", 48, 21, 44, 80, 3072, True, (0, 1)),
         ("96", 96, 21, 60, 104, 1536, False, (0, 1)))
for name, C, F, H, W, D, first, paths in CASES:
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, C, F, H, W, generator=g).cuda()
    ff = torch.randn(1, C, 1, H, W, generator=g).cuda() if first else None
    w = (torch.randn(D, C * 4, generator=g) * (4 * C) ** -0.5).cuda()
    b = torch.randn(D, generator=g).cuda()
    tok = torch.empty(F * (H // 2) * (W // 2), D, dtype=torch.bfloat16, device="cuda")
    for path in paths:
        if C > 64:
            fn = lambda: _lib.check(L.fg_op_wan_vace_patch_embed(ptr(x), ptr(w), ptr(b), ptr(tok), 1, C, F, H, W, D, path, None))  # noqa: E731
        else:
            fn = lambda: _lib.check(L.fg_op_wan_patch_embed(ptr(x), ptr(ff), ptr(w), ptr(b), ptr(tok), 1, C, F, H, W, D, path, None))  # noqa: E731
        med, lo, hi = timeit(fn)
        print(json.dumps({"case": name, "path": path, "us_median": round(med, 2), "us_min": round(lo, 2), "us_max": round(hi, 2)}), flush=True)
