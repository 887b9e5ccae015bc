"""The output head of the Wan2.2-TI2V-5B network on its own (fastgen_amd/csrc/wan_ti2v.hip) at the 5B shape [1, 48, 21, 44, 80], D 3072:
the tiled 48-channel head (path 2) against the wave-per-token head of wan.hip on the same inputs (path 1), through fg_op_wan_final, with
and without the first-frame source.  us per launch from device events, median / min / max of 10 launches after 3 warm-ups.  (The patch
embedding: scripts/wan_embed_bench.py.)
    python scripts/wan_ti2v_ops_bench.py"""
import torch

from fastgen_amd import _lib
from fastgen_amd.networks._engine import ptr

B, C, F, H, W, D = 1, 48, 21, 44, 80, 3072
L = _lib.lib()
g = torch.Generator().manual_seed(0)
ff = torch.randn(B, C, 1, H, W, generator=g).cuda()
ntok = B * F * (H // 2) * (W // 2)
tok = torch.randn(ntok, D, generator=g).bfloat16().cuda()
mod = (0.5 * torch.randn(B * F, 2, D, generator=g)).cuda()
wo = (torch.randn(4 * C, D, generator=g) * D ** -0.5).cuda()
bo = torch.randn(4 * C, generator=g).cuda()
out = torch.empty(B, C, F, H, W, device="cuda")


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


res = {}
for name, src in (("plain", None), ("first_frame", ff)):
    for path in (2, 1):
        fn = lambda: _lib.check(L.fg_op_wan_final(ptr(tok), ptr(mod), ptr(wo), ptr(bo), ptr(src), ptr(out), B, C, F, H // 2, W // 2, D, 1e-6, path, None))
        res[(name, path)] = timeit(fn)
        print("final", name, "path", path, "us median/min/max", res[(name, path)], flush=True)
for name in ("plain", "first_frame"):
    print("final", name, "ratio old/new", res[(name, 1)][0] / res[(name, 2)][0])
