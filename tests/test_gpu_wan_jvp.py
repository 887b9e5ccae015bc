"""`fg_wan_jvp` / `Wan.jvp` (fastgen_amd/csrc/engine_wan_jvp.inc, kernels wan_jvp.hip + the bf16 token GEMM) against the fp64 tangent
`torch.func.jvp` over tests/wan_jvp_ref.py::forward_rows (the composition of oracle/wan_ref.py's pieces that tests/test_wan_jvp_ref.py
pins to `WanFullRef.forward`), through the C ABI on 2-layer networks (J.NET_CASES: 2 heads, ffn 512, 37 text tokens; Q_GAIN on norm_q).
EVERY FRAME HAS ITS OWN t, r, vt AND vr (J.frame_rows: none coincide, t - r > 0), as in tests/test_gpu_wan_full_blocks.py: the module
only ever hands the engine one value per sample, so an engine that indexed a tangent per sample would pass every module-level test.

Cases: 7 frames x 15 tokens (with and without the r_embedder), 5 x 96 tokens at B 2 under "diff" and "abs", 12 x 96 tokens at B 2
(1152 tokens; the oracle runs on the device), width 1536 at 105 tokens.  Directions: x = (v_x, 0, 0) with null vt / vr pointers,
t = (0, 1, 0) (rows of 1000: the derivative of the x1000 timestep scale on v_t = 1), all = (v_x, vt, vr) with per-frame rows.
Per sample: relative L2 and max |err| / max |ref| of the tangent (NET_TOL); `out` against the fp64 forward under the bound
tests/test_gpu_wan_full.py uses (2e-2) and against fg_wan_forward_full on the same inputs (OUT_VS_FORWARD, twice the worst measured:
the two are not bit-equal - the jvp's GELU runs on the stored bf16 pre-activation and its attention kernel is its own); a second call returns the same bits; rows 1:3 of a B 4 call equal a B 2 call bit for bit.

Mutants (tests/wan_jvp_ref.py, built in fp64 from the mirror alone) in the direction `all`: each one outside J.NET_WEAK_MUTANTS must
miss NET_TOL MUTANT_FACTOR times over in its closest sample; tests/test_wan_jvp_ref.py::test_network_mutants_stand_apart shows their
distances from the reference on the CPU, and the per-op file sees the weak ones."""
import ctypes

import pytest
import torch

import wan_jvp_ref as J
from fastgen_amd import _lib
from test_gpu_wan_blocks import MUTANT_FACTOR

pytestmark = pytest.mark.gpu

OUT_TOL = 2e-2          # tests/test_gpu_wan_full.py's TOL: `out` against the fp64 forward, relative L2 per sample
OUT_VS_FORWARD = 7.3e-3  # `out` against fg_wan_forward_full on the same inputs: twice the worst measured on an MI355X, 3.65e-3 (F1152)
DIRECTIONS = ("x", "t", "all")


def dev():
    return torch.device("cuda:0")


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Gpu:
    """The engine behind `Wan`, called through the C ABI (as tests/test_gpu_wan_blocks.py::Gpu)."""

    def __init__(self, name, batch=None, compute_dtype=None):
        from fastgen_amd.networks.Wan.network import Wan

        c = J.NET_CASES[name]
        cfg, sd, _ = J.net_case_weights(name)
        net = Wan(num_attention_heads=cfg.num_heads, attention_head_dim=128, in_channels=16, out_channels=16, text_dim=cfg.text_dim,
                  ffn_dim=cfg.ffn_dim, num_layers=cfg.num_layers, rope_max_seq_len=cfg.rope_max_seq_len, r_timestep=bool(c["r"]),
                  time_cond_type=c["r"] or "diff", compute_dtype=compute_dtype)
        net.load_state_dict(sd, strict=True)
        self.net = net.to(dev()).eval()
        self.net._bind(dev())
        self.h, self.L = self.net._h, _lib.lib()
        self.B, self.Fr, self.lat = batch or c["B"], c["frames"], c["lat"]
        self.stream = ctypes.c_void_p(torch.cuda.current_stream(dev()).cuda_stream)
        self.need = self.L.fg_wan_jvp_workspace_bytes(self.h, self.B, self.Fr, *self.lat)
        full = self.L.fg_wan_full_workspace_bytes(self.h, self.B, self.Fr, *self.lat)
        self.ws = torch.empty(max(self.need, full, 256), dtype=torch.uint8, device=dev())

    def set_text(self, text):
        self.text = text.float().to(dev()).contiguous()
        _lib.check(self.L.fg_wan_set_text(self.h, _p(self.text), self.B, self.text.shape[1], _p(self.ws), self.ws.numel(), self.stream))

    @staticmethod
    def _f32(v):
        return None if v is None else v.float().to(dev()).contiguous()

    def args(self, x, ts, rs, vx, vts, vrs, out=None, jv=None, ws_bytes=None, skip=None):
        self.keep = [self._f32(v) for v in (x, ts, rs, vx, vts, vrs)]
        xg, tg, rg, vxg, vtg, vrg = self.keep
        out = torch.full_like(xg, float("nan")) if out is None else out
        jv = torch.full_like(xg, float("nan")) if jv is None else jv
        sk = (ctypes.c_int * len(skip))(*skip) if skip else None
        return out, jv, (self.h, _p(xg), _p(tg), _p(rg), _p(vxg), _p(vtg), _p(vrg), _p(out), _p(jv), self.B, self.Fr, self.lat[0], self.lat[1],
                         sk, len(skip) if skip else 0, _p(self.ws), self.need if ws_bytes is None else ws_bytes, self.stream)

    def jvp(self, x, ts, rs, vx, vts, vrs):
        out, jv, a = self.args(x, ts, rs, vx, vts, vrs)
        _lib.check(self.L.fg_wan_jvp(*a))
        torch.cuda.synchronize()
        return out, jv

    def forward(self, x, ts, rs):
        xg, tg, rg = self._f32(x), self._f32(ts), self._f32(rs)
        out = torch.full_like(xg, float("nan"))
        _lib.check(self.L.fg_wan_forward_full(self.h, _p(xg), _p(tg), _p(rg), _p(out), self.B, self.Fr, self.lat[0], self.lat[1], None, 0,
                                              _p(self.ws), self.ws.numel(), self.stream))
        torch.cuda.synchronize()
        return out

    def close(self):
        del self.net, self.ws
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def _tangents(d, vx, vts, vrs):
    """(engine arguments, oracle arguments) of direction d."""
    z = torch.zeros_like
    if d == "x":
        return (vx, None, None), (vx, z(vts), None if vrs is None else z(vrs))
    if d == "t":
        ones = torch.full_like(vts, 1000.0)
        return (z(vx), ones, None), (z(vx), ones, None if vrs is None else z(vrs))
    return (vx, vts, vrs), (vx, vts, vrs)


def _err(got, ref):
    dims = tuple(range(1, ref.ndim))
    e = got - ref
    return e.pow(2).sum(dims).sqrt() / ref.pow(2).sum(dims).sqrt(), e.abs().amax(dims) / ref.abs().amax(dims)


@pytest.mark.parametrize("name", list(J.NET_CASES))
def test_jvp_against_fp64(name):
    c = J.NET_CASES[name]
    odev = dev() if c.get("device") else torch.device("cpu")
    cfg, p, x, ts, rs, vts, vrs, text, vx = J.net_case(name, odev)
    diff = c["r"] == "diff"
    gpu = Gpu(name)
    bad = []
    try:
        gpu.set_text(text)
        fwd = gpu.forward(x, ts, rs).double().to(odev)
        for d in DIRECTIONS:
            eng, orc = _tangents(d, vx, vts, vrs)
            out, jv = gpu.jvp(x, ts, rs, *eng)
            with torch.no_grad():
                want, wantd = J.oracle_jvp(p, cfg, x, ts, rs, text, *orc, diff)
            rel, mx = _err(jv.double().to(odev), wantd)
            print(f"[wan-jvp] {name} {d}: jvp {float(rel.max()):.3e} / {float(mx.max()):.3e}  (bound {J.NET_TOL[0]:.2e} / {J.NET_TOL[1]:.2e})")
            if not (bool((rel <= J.NET_TOL[0]).all()) and bool((mx <= J.NET_TOL[1]).all())):
                bad.append((d, "jvp", rel.tolist(), mx.tolist()))
            ro, rf = _err(out.double().to(odev), want)[0], _err(out.double().to(odev), fwd)[0]
            print(f"[wan-jvp] {name} {d}: out vs fp64 {float(ro.max()):.3e}, vs fg_wan_forward_full {float(rf.max()):.3e}")
            if not (bool((ro <= OUT_TOL).all()) and bool((rf <= OUT_VS_FORWARD).all())):
                bad.append((d, "out", ro.tolist(), rf.tolist()))
            if d == "all":
                out2, jv2 = gpu.jvp(x, ts, rs, *eng)
                if not (torch.equal(out, out2) and torch.equal(jv, jv2)):
                    bad.append("a second call returns other bits")
                with torch.no_grad():
                    for m in J.MUTANTS:
                        if (m == "flip_vr" and rs is None) or m in J.NET_WEAK_MUTANTS:
                            continue
                        dist = float(J.rel_l2(jv.double().to(odev), J.mutant_jvp(m, p, cfg, x, ts, rs, text, vx, vts, vrs, diff)).min())
                        print(f"[wan-jvp] {name} mutant {m}: closest sample {dist:.3e} = {dist / J.NET_TOL[0]:.1f} x bound")
                        if not dist >= MUTANT_FACTOR * J.NET_TOL[0]:
                            bad.append(("mutant not seen", m, dist / J.NET_TOL[0]))
    finally:
        gpu.close()
    assert not bad, bad


def test_rows_of_a_larger_batch():
    """Rows 1:3 of a B 4 call equal the B 2 call on those samples bit for bit."""
    name = "F480-diff"
    _, _, x, ts, rs, vts, vrs, text, vx = J.net_case(name, batch=4)
    big = Gpu(name, batch=4)
    try:
        big.set_text(text)
        o4, j4 = big.jvp(x, ts, rs, vx, vts, vrs)
    finally:
        big.close()
    small = Gpu(name, batch=2)
    try:
        small.set_text(text[1:3])
        o2, j2 = small.jvp(x[1:3], ts[1:3], rs[1:3], vx[1:3], vts[1:3], vrs[1:3])
    finally:
        small.close()
    assert torch.equal(o4[1:3], o2) and torch.equal(j4[1:3], j2)


def test_refusals_launch_nothing():
    FG_EINVAL, FG_ENOMEM = 1, 4
    name = "F105"
    _, _, x, ts, rs, vts, vrs, text, vx = J.net_case(name)
    gpu = Gpu(name)
    try:
        gpu.set_text(text)
        L = gpu.L

        def refused(code, word, **kw):
            out, jv, a = gpu.args(x, ts, rs, vx, vts, vrs, **kw)
            assert L.fg_wan_jvp(*a) == code and word in L.fg_last_error(), (kw, L.fg_last_error())
            torch.cuda.synchronize()
            return out, jv

        for kw, code, word in ((dict(skip=(0,)), FG_EINVAL, b"skip_layers"), (dict(ws_bytes=gpu.need - 1), FG_ENOMEM, b"workspace")):
            out, jv = refused(code, word, **kw)
            assert bool(out.isnan().all()) and bool(jv.isnan().all()), kw
        for idx in (7, 8):  # out, then jvp, on x_t itself
            _, _, a = gpu.args(x, ts, rs, vx, vts, vrs)
            a = list(a)
            a[idx] = a[1]
            before = gpu.keep[0].clone()
            assert L.fg_wan_jvp(*a) == FG_EINVAL and b"alias" in L.fg_last_error()
            torch.cuda.synchronize()
            assert torch.equal(gpu.keep[0], before)
        assert L.fg_wan_jvp(*gpu.args(x, ts, rs, vx, vts, vrs)[2]) == 0  # (and the good call still runs)
    finally:
        gpu.close()
    # handles of the networks without a tangent, through the C ABI: refused on the handle's kind, before anything else is looked at
    xg = Gpu._f32(x)
    fake = torch.zeros(64, device=dev())
    for kind, word in (("i2v", b"image-to-video"), ("vace", b"VACE")):
        h = J.make_handle(kind=kind)
        try:
            L = _lib.lib()
            assert L.fg_wan_jvp_workspace_bytes(h, 1, 7, 10, 6) == 0
            out, jv = torch.full_like(xg, float("nan")), torch.full_like(xg, float("nan"))
            assert L.fg_wan_jvp(h, _p(xg), _p(fake), None, _p(xg), None, None, _p(out), _p(jv), 1, 7, 10, 6, None, 0, _p(fake), 1 << 30,
                                None) == FG_EINVAL and word in L.fg_last_error()
            torch.cuda.synchronize()
            assert bool(out.isnan().all()) and bool(jv.isnan().all())
        finally:
            L.fg_wan_destroy(h)
    fp8 = Gpu(name, compute_dtype="fp8")
    try:
        assert fp8.need == 0
        out, jv, a = fp8.args(x, ts, rs, vx, vts, vrs, ws_bytes=1 << 30)
        assert fp8.L.fg_wan_jvp(*a) == FG_EINVAL and b"fp8" in fp8.L.fg_last_error()
        torch.cuda.synchronize()
        assert bool(out.isnan().all()) and bool(jv.isnan().all())
        with pytest.raises(NotImplementedError, match="no forward-mode derivative"):
            fp8.net.jvp(fp8._f32(x), torch.tensor([0.5], device=dev()), fp8._f32(vx), condition=fp8._f32(text), r=torch.tensor([0.2], device=dev()))
    finally:
        fp8.close()


def test_module_jvp_and_meanflow():
    """`Wan.jvp` and `MeanFlowModel.network_jvp(Wan)` with the reference's tangents (dxt_dt, 1, 0) against the oracle tangent: one t and r
    per sample, `rescale_t` and its derivative inside the module.  Beside it, printed once and not asserted: the central difference of
    two `Wan.forward` calls at the reference's jvp_finite_diff_eps = 5e-3 (configs/experiments/WanT2V/config_mf.py) against the same
    fp64 tangent - the alternative this feature replaces."""
    from fastgen_amd.methods.consistency_model.mean_flow import MeanFlowModel

    name = "F480-diff"
    cfg, p, x, _, _, _, _, text, vx = J.net_case(name)
    t, r = torch.tensor([0.8, 0.45], dtype=torch.float64), torch.tensor([0.3, 0.1], dtype=torch.float64)
    Fr = x.shape[2]
    rows = lambda v: (1000.0 * v.float()).double().view(2, 1).expand(2, Fr).contiguous()  # noqa: E731
    one, zero = torch.ones(2, dtype=torch.float64), torch.zeros(2, dtype=torch.float64)
    with torch.no_grad():
        want, wantd = J.oracle_jvp(p, cfg, x, rows(t), rows(r), text, vx, rows(one), rows(zero), True)
    gpu = Gpu(name)
    try:
        net = gpu.net
        g = lambda v: v.float().to(dev())  # noqa: E731
        with torch.no_grad():
            out, jv = net.jvp(g(x), g(t), g(vx), g(one), condition=g(text), r=g(r), v_r=g(zero))
            mf = MeanFlowModel.network_jvp(net, g(x), g(t), g(r), g(vx), condition=g(text))
            eps = 5e-3
            cd = (net(g(x + eps * vx), g(t + eps), condition=g(text), r=g(r)) - net(g(x - eps * vx), g(t - eps), condition=g(text), r=g(r))) / (2 * eps)
        assert torch.equal(mf, jv) and out.dtype == torch.float32
        rel, mx = _err(jv.double().cpu(), wantd)
        print(f"[wan-jvp] module {name}: jvp {float(rel.max()):.3e} / {float(mx.max()):.3e}; out {float(_err(out.double().cpu(), want)[0].max()):.3e}")
        print(f"[wan-jvp] module {name}: central difference of Wan.forward at eps 5e-3: {float(_err(cd.double().cpu(), wantd)[0].max()):.3e}")
        assert bool((rel <= J.NET_TOL[0]).all()) and bool((mx <= J.NET_TOL[1]).all()), (rel, mx)
        assert bool((_err(out.double().cpu(), want)[0] <= OUT_TOL).all())
        bf = net.jvp(g(x).bfloat16(), g(t), g(vx).bfloat16(), g(one), condition=g(text), r=g(r))
        assert bf[0].dtype == torch.bfloat16 and bf[1].dtype == torch.bfloat16
    finally:
        gpu.close()
