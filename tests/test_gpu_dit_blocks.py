"""Per-block and per-op parity of the DiT kernels (fastgen_amd/csrc/dit.hip, engine_dit.inc, the token GEMMs of gemm.hip / conv.hip,
wan.hip's whole-sequence head-dim-72 attention) against the oracle (oracle/dit_ref.py) in fp64, sample by sample, on every path the
library takes: S/2, B/2, L/2, XL/2 at their real widths (depth 2 or 3: the kernels do not depend on depth, and two blocks make the
offsets of the stacked modulation GEMM matter), fp32 / bf16x3 / bf16, batches that straddle the groups of 8 of the sample-major
attention mapping, the stacked modulation GEMM (bf16, B >= 256) and the row cutting of the split-bf16 GEMM (B = 512 at XL), patch 1 / 2 / 4,
3 latent channels, 10 classes; and the environment switches that move the linears and the attention onto other kernels.

`fg_dit_forward_features` with every block tapped hands back each block's output tokens as fp32: exactly what the next block consumed
(fp32 storage in fp32 / bf16x3, bf16 widened in bf16).  So each block is run by the oracle on the GPU's own input (block 0: the oracle's
patch embedding) and conditioning vector (`cond_out`, itself pinned against the oracle), and what is compared is the block's INCREMENT
(tap[i] - tap[i-1] against ref_i - tap[i-1]): the residual stream would hide a wrong attention or MLP branch.  Every sample has its own
x, t (r) and class (one row unconditional); at B >= 9 a handful of samples is fetched and checked.

Bounds (relative L2 and max |error| / max |reference|, the worst measured value in the commit message that set them): see TOL.  Two
checks show they discriminate: bf16 increments fail the bf16x3 bound, and a sample's reference against its neighbour's GPU increment
fails every bound many times over (the check sees cross-sample mixing)."""
import ctypes
import os

import pytest
import torch

from fastgen_amd import _lib
from oracle import dit_ref as R

pytestmark = pytest.mark.gpu

_S = dict(hidden_size=384, num_heads=6)
ARCH = {
    "S": dict(_S, depth=3),
    "B": dict(hidden_size=768, num_heads=12, depth=2),
    "L": dict(hidden_size=1024, num_heads=16, depth=2),
    "XL": dict(hidden_size=1152, num_heads=16, depth=2),
    "XLr": dict(hidden_size=1152, num_heads=16, depth=2, r_timestep=True),
    "Sp4": dict(_S, depth=2, input_size=64, patch_size=4),
    "Sp1": dict(_S, depth=2, input_size=16, patch_size=1),
    "Sc3": dict(_S, depth=2, in_channels=3),
    "Snc10": dict(_S, depth=2, num_classes=10),
}

CASES = ([("S", m, b) for m in ("fp32", "bf16x3", "bf16") for b in (1, 3, 9, 256)]
         + [(a, m, b) for a in ("B", "L") for m in ("bf16x3", "bf16") for b in (3, 256)]
         + [("XL", m, b) for m in ("fp32", "bf16x3", "bf16") for b in (1, 3, 9, 255, 256, 257)]
         + [("XL", "bf16x3", 512)]
         + [(a, m, 3) for a in ("XLr", "Sp4", "Sp1", "Sc3", "Snc10") for m in ("bf16x3", "bf16")])

# (relative L2, max |err| / max |ref|) of: c, a block's increment, the final layer's output.  Worst measured on an MI355X over the
# matrix (switch paths included): c 6.3e-6 / 6.2e-6; increments fp32 1.4e-6 / 3.7e-6, bf16x3 6.6e-6 / 1.0e-5, bf16 1.25e-2 / 1.9e-2;
# out 4.3e-7 / 4.3e-7 (the final layer computes in fp32 in every mode, on the tokens the GPU's last block left)
TOL = {
    "fp32": dict(c=(2.5e-5, 2.5e-5), inc=(5e-6, 1.5e-5), out=(1.5e-6, 1.5e-6)),
    "bf16x3": dict(c=(2.5e-5, 2.5e-5), inc=(2.5e-5, 4e-5), out=(1.5e-6, 1.5e-6)),
    "bf16": dict(c=(2.5e-5, 2.5e-5), inc=(2.5e-2, 5e-2), out=(1.5e-6, 1.5e-6)),
}
LOOSEST = tuple(max(TOL[m][k][j] for m in TOL for k in ("inc", "out")) for j in (0, 1))

_NETS = {}


def _net(arch):
    """One module (engines per compute dtype inside) and its fp64 state dict per architecture."""
    if arch not in _NETS:
        from fastgen_amd.networks.DiT.network import DiT

        cfg = R.DiTConfig(**ARCH[arch])
        sd = R.random_state_dict(cfg, seed=1000 + list(ARCH).index(arch))
        net = DiT(**ARCH[arch])
        net.load_state_dict(sd, strict=True)
        _NETS.clear()  # one architecture's engines at a time
        _NETS[arch] = (net.to("cuda:0").eval(), cfg, {k: v.double() for k, v in sd.items()})
    return _NETS[arch]


def _checked(B):
    if B < 9:
        return list(range(B))
    s = {0, 1, 8 if B < 14 else 13, B // 2, B - 1}
    if B == 512:
        s |= {454, 455, 456}  # the fc2 launch of the split-bf16 GEMM is cut at image 455 (2^31 / (4 * 4608) rows)
    return sorted(s)


def _inputs(cfg, B, seed):
    """x, t (and r < t) and a class of its own per sample; sample 1 is the unconditional row."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, cfg.in_channels, cfg.input_size, cfg.input_size), generator=g)
    t = (0.02 + 0.96 * torch.rand(B, generator=g, dtype=torch.float64))
    r = t * torch.rand(B, generator=g, dtype=torch.float64) if cfg.r_timestep else None
    reps = (B + cfg.num_classes - 1) // cfg.num_classes
    cls = torch.cat([torch.randperm(cfg.num_classes, generator=g) for _ in range(reps)])[:B]
    if B > 1:
        cls[1] = cfg.num_classes
    return x, t, r, cls


def _run(net, mode, x, t, r, cls, rows):
    """fg_dit_forward_features with every block tapped and cond_out: (c, [tap_i], out) of the samples `rows`, on the CPU in fp64."""
    dev = torch.device("cuda:0")
    net.compute_dtype = mode
    dt, h = net._engine(dev)
    L = _lib.lib()
    B, depth, D = x.shape[0], net._cfg.depth, net.hidden_size
    xd = x.to(dev).contiguous()
    te = net.prepare_t(t.to(dev), torch.float32).contiguous()
    re = net.prepare_t(r.to(dev), torch.float32).contiguous() if r is not None else None
    cd = cls.to(dev)
    out = torch.empty_like(xd)
    cond = torch.empty(B, D, device=dev)
    taps = [torch.empty(B, 256, D, device=dev) for _ in range(depth)]
    need = L.fg_dit_workspace_bytes(h, B)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    p = lambda v: ctypes.c_void_p(v.data_ptr()) if v is not None else None  # noqa: E731
    _lib.check(L.fg_dit_forward_features(h, p(xd), p(te), p(re), p(cd), p(out), p(cond), (ctypes.c_int * depth)(*range(depth)),
                                         (ctypes.c_void_p * depth)(*[f.data_ptr() for f in taps]), depth, B, p(ws), need,
                                         ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    idx = torch.tensor(rows, device=dev)
    res = (cond[idx].double().cpu(), [f[idx].double().cpu() for f in taps], out[idx].double().cpu(), te[idx].double().cpu(),
           None if re is None else re[idx].double().cpu())
    del taps, ws, out, cond
    torch.cuda.synchronize()
    return res


def _err(got, ref, base):
    """(relative L2, max |err| / max |ref - base|) of got against ref, per sample (dim 0)."""
    e = (got - ref).flatten(1)
    d = (ref - base).flatten(1)
    return (e.norm(dim=1) / d.norm(dim=1)).tolist(), (e.abs().amax(dim=1) / d.abs().amax(dim=1)).tolist()


def _check(what, mode, rows, rel, mx, worst, bad):
    bound = TOL[mode][what]
    worst[what] = max(worst.get(what, (0.0, 0.0))[0], max(rel)), max(worst.get(what, (0.0, 0.0))[1], max(mx))
    bad += [(what, s, rel[j], mx[j]) for j, s in enumerate(rows) if not (rel[j] <= bound[0] and mx[j] <= bound[1])]


@pytest.mark.parametrize("arch,mode,B", CASES, ids=[f"{a}-{m}-B{b}" for a, m, b in CASES])
def test_blocks(arch, mode, B):
    net, cfg, sd = _net(arch)
    rows = _checked(B)
    x, t, r, cls = _inputs(cfg, B, seed=17 * B + len(arch))
    c_gpu, taps, out, te, re = _run(net, mode, x, t, r, cls, rows)
    x, cls = x[rows].double(), cls[rows]
    worst, bad = {}, []  # (every check runs: a failure names all the blocks and samples it reaches)
    with torch.no_grad():
        # c = t_emb + y_emb (+ r_emb): fourier_kernel, the embedder linears, cond_kernel (on the timesteps the kernels read)
        c_ref = R.time_embedding(sd, "t_embedder", te) + sd["y_embedder.class_embeddings.weight"][cls]
        if re is not None:
            c_ref = c_ref + R.time_embedding(sd, "r_embedder", re)
        _check("c", mode, rows, *_err(c_gpu, c_ref, 0.0), worst, bad)
        # every block on the GPU's own input and conditioning vector; block 0 after the oracle's patch embedding
        prev = R.patch_embed(sd, cfg, x)
        for i, tap in enumerate(taps):
            ref = R.dit_block(sd, i, prev, c_gpu, cfg.num_heads)
            rel, mx = _err(tap, ref, prev)
            _check("inc", mode, rows, rel, mx, worst, bad)
            if mode == "bf16":  # the bound of the split-bf16 mode tells the bf16 mode apart
                bad += [("bf16 within the bf16x3 bound", i, v) for v in rel if not v > TOL["bf16x3"]["inc"][0]]
            if len(rows) > 1:  # sample j's reference against sample j + 1's GPU increment: mixing samples is seen
                xr, xm = _err((tap - prev)[1:], (ref - prev)[:-1], 0.0)
                worst["cross"] = min(worst.get("cross", (1e9, 1e9))[0], min(xr)), min(worst.get("cross", (1e9, 1e9))[1], min(xm))
                if not (min(xr) > 20 * LOOSEST[0] and min(xm) > 5 * LOOSEST[1]):
                    bad.append(("cross-sample check blind", i, xr, xm))
            prev = tap
        _check("out", mode, rows, *_err(out, R.final_layer(sd, cfg, prev, c_gpu), 0.0), worst, bad)
    print(f"\n[dit-blocks] {arch}-{mode}-B{B} " + " ".join(f"{k}={v[0]:.2e}/{v[1]:.2e}" for k, v in worst.items()))
    assert not bad, bad


@pytest.mark.parametrize("env,select", [
    ("FASTGEN_AMD_DIT_GEMM", "S-bf16-B or XL-bf16-B"),                  # bf16 linears on conv.hip's token modes; XL: dit_attention_kernel<__bf16, 72>
    ("FASTGEN_AMD_DIT_GEMM3", "S-bf16x3-B or XL-bf16x3-B"),              # bf16x3 linears on conv.hip's token modes
    ("FASTGEN_AMD_FA_SEQ72", "XL-bf16-B"),                               # DiT-XL bf16 attention on fa_kernel<72>
])
def test_switch_paths(env, select):
    """The switches are read once per process: the S/2 and XL/2 cases they affect run again in a child process with the switch at 0."""
    import subprocess
    import sys

    if os.environ.get(env) == "0":
        pytest.skip(f"already running with {env}=0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k",
                        f"test_blocks and ({select})"], env=dict(os.environ, **{env: "0"}), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and " failed" not in r.stdout, r.stdout[-2000:]
