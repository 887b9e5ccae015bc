"""Per-op, per-element parity of the SongUNet (EDMPrecond) INFERENCE kernels - conv_fused_kernel in every instantiation of launch_t,
conv3_ws_kernel, conv3_x3ws_kernel (RES_SUBPIX and rshift included), gn_finalize_kernel, gn_silu_pool_kernel, stem_kernel,
conv_in_kernel, aux_head_kernel, aux_out_kernel, the three attention kernels, attn_merge_weights_kernel and the merged attention -
through the fg_op_edm_* entry points over their launchers, each against the plain fp64 reference of tests/edm_ops_ref.py:
|got - ref| <= bound for EVERY element, in the three compute modes.  The plan (which kernel, how many statistics slots) is asserted
before each conv, so "this case reached conv3_ws_kernel" is a checked fact; every wave-specialised case also runs on conv_fused_kernel
(wpack_ws = NULL).  Outputs and statistics are pre-filled with NaN, every source tensor sits inside a larger allocation whose guard
regions are NaN, and the gap of the pitched temb is NaN: an element not written, an unmasked halo or a past-the-batch read fails.  Every
launch is made twice and must be bit-identical.  tests/test_edm_ops_ref.py shows on the CPU that these inputs reject the named mutations.

Each check prints `HEADROOM <op> <mode> <case> <output> <worst |err| / bound>` and the mean-offset cases `OFFSET <mode> <offset>
<worst error of the normalised value> <its bound>` (DESIGN.md's tables).

Measured on an MI355X, worst |err| / bound over the cases as fp32 / bf16 / bf16x3 (1.000 = exactly half an ulp of the store off; the
same table is in DESIGN.md, "The SongUNet inference kernels pinned per op and per element"):
    conv_fused_kernel out, q, k, vt 0.169 / 0.999 / 0.466, statistics 0.014 / 0.016 / 0.013
    conv3_ws_kernel (bf16) out 1.000, statistics 0.011;  conv3_x3ws_kernel (bf16x3) out 0.112, statistics 0.043
    gn_finalize ab, mr 1.000 / 0.982 / 0.996;  gn_silu_pool 0.392 / 1.000 / 0.412
    stem out 0.317 / 1.000 / 0.316, statistics 0.021 / 0.016 / 0.024;  conv_in 0.317 / 1.000 / 0.316
    aux_head 0.007 / 0.073 / 0.011;  aux_out 0.002 / 0.002 / 0.002;  attention 0.037 / 0.997 / 0.082
    attn_merge_weights 0.998;  attention_merged (bf16x3) out 0.012, statistics 0.021
Before conv3_ws_kernel and stem_kernel were changed to sum the values as stored, the bf16 statistics of conv3_ws_kernel missed the bound
(c3_128_32_b3: 2 808 of 3 072 slot entries, worst 4.3e-3 relative against 3e-5)."""
import ctypes
import functools

import pytest
import torch

from fastgen_amd import _lib

import edm_ops_ref as R

pytestmark = pytest.mark.gpu

F64 = torch.float64
NAN = float("nan")
GUARD = 4096  # elements of NaN on either side of a guarded tensor
MODE_IDS = R.MODE_NAME.get


def dev():
    return torch.device("cuda:0")


def tdt(mode):
    return torch.bfloat16 if mode == 1 else torch.float32


def guarded(t, dtype):
    """fp64 values -> a device tensor of `dtype` in the middle of a larger NaN-filled allocation (16-byte aligned)."""
    if t is None:
        return None
    buf = torch.full((t.numel() + 2 * GUARD,), NAN, dtype=dtype, device=dev())
    view = buf[GUARD:GUARD + t.numel()].view(t.shape)
    view.copy_(t.to(dtype))
    return view


def f32(t):
    return None if t is None else t.to(torch.float32).contiguous().to(dev())


def nans(shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=dev())


def ptr(t):
    return None if t is None else t.data_ptr()


def back(t):
    torch.cuda.synchronize()
    return t.detach().cpu().to(F64)


def same_bits(a, b):
    torch.cuda.synchronize()
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def check(tag, got, ref, bound):
    assert got.shape == ref.shape == bound.shape, (tag, got.shape, ref.shape, bound.shape)
    assert torch.isfinite(got).all(), f"{tag}: {(~torch.isfinite(got)).sum().item()} elements NaN (not written, or fed by a guard region)"
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    worst = ratio.max().item()
    print(f"HEADROOM {tag} {worst:.4f}")
    if worst > 1.0:
        i = ratio.argmax().item()
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
        raise AssertionError(f"{tag}: {(ratio > 1).sum().item()} of {ratio.numel()} elements outside the bound; worst at {idx}: got "
                             f"{got.flatten()[i].item():.9g}, ref {ref.flatten()[i].item():.9g}, bound {bound.flatten()[i].item():.3g}")


def call(rc):
    _lib.check(rc)


# ---- the conv ----------------------------------------------------------------------------------------------------------------------------

def conv_plan(d, mode, ws):
    p = _lib.fg_edm_conv_plan()
    call(_lib.lib().fg_op_edm_conv_plan(mode, d["ks"], d["pro"], d["res"], d["outmode"], d["c1"], d["c2"], d["B"], d["hs"], d["h"], d["cout"], int(ws),
                                        d["rshift"], ctypes.byref(p)))
    return p.kernel, p.stat_slots


def pack(w, mode, layout, ks, qkv_perm=False):
    L = _lib.lib()
    cout, cin = w.shape[0], w.shape[1]
    n = L.fg_op_edm_conv_pack_bytes(mode, layout, cout, cin, ks)
    assert n > 0, (mode, layout, cout, cin, ks)
    out = torch.empty(n, dtype=torch.uint8, device=dev())
    wd = f32(w)
    call(L.fg_op_edm_conv_pack(mode, layout, wd.data_ptr(), out.data_ptr(), cout, cin, ks, int(qkv_perm), None))
    torch.cuda.synchronize()
    return out


def run_conv(d, mode, ws):
    """One case through fg_op_edm_conv, twice: ({output name: fp64 CPU tensor}, stats [B, S, cout / 4, 2] or None, (kernel, slots))."""
    L = _lib.lib()
    B, h, cout, T = d["B"], d["h"], d["cout"], tdt(mode)
    wp = pack(d["w"], mode, _lib.FG_EDM_PACK_GENERIC, d["ks"], d["qkv_perm"])
    wws = None
    if ws:
        layout = _lib.FG_EDM_PACK_X3SUB if d["res"] == R.RES_SUBPIX else (_lib.FG_EDM_PACK_WS if mode == 1 else _lib.FG_EDM_PACK_X3WS)
        wws = pack(d["w"], mode, layout, 3)
    kernel, slots = conv_plan(d, mode, ws)
    src1, src2, resid = guarded(d["src1"], T), guarded(d["src2"], T), guarded(d["resid"], T)
    ab, bias = guarded(d["ab"], torch.float32), guarded(d["bias"], torch.float32)
    temb, stride = None, 0
    if d["temb"] is not None:  # pitched rows, NaN in the gap
        stride = cout + 32
        temb = nans((B, stride))
        temb[:, :cout] = f32(d["temb"])
    nhwc = d["outmode"] == R.OUT_NHWC
    runs = []
    for _ in range(2):
        o = dict(out=nans((B, h, h, cout), T) if nhwc else None, stats=nans((B, slots, cout // 4, 2)) if nhwc else None,
                 q=None if nhwc else nans((B, h * h, 256), T), k=nans((B, h * h, 256), T) if d["outmode"] == R.OUT_QKV else None,
                 vt=None if nhwc else nans((B, 256, h * h), T))
        call(L.fg_op_edm_conv(mode, d["ks"], d["pro"], d["res"], d["outmode"], ptr(src1), d["c1"], ptr(src2), d["c2"], B, d["hs"], h, ptr(ab), ptr(wp), ptr(wws),
                              ptr(bias), ptr(temb), stride, ptr(resid), d["rshift"], d["scale"], ptr(o["out"]), cout, ptr(o["stats"]), ptr(o["q"]), ptr(o["k"]),
                              ptr(o["vt"]), None))
        runs.append(o)
    for key in runs[0]:
        if runs[0][key] is not None:
            assert same_bits(runs[0][key], runs[1][key]), f"{d['name']} {key}: two launches differ"
    outs = {k: back(v) for k, v in runs[0].items() if v is not None and k != "stats"}
    return outs, (back(runs[0]["stats"]) if nhwc else None), (kernel, slots)


@functools.lru_cache(maxsize=None)
def conv_ref(name, mode):
    d = R.conv_inputs(name, mode)
    return d, R.conv(d, mode)


def check_stats_and_finalize(tag, out, stats, layout, hw):
    """The slots against the fp64 sums of the tensor as stored, then gn_finalize on the device's own slots against its reference."""
    sv, sb = R.slot_stats(out, layout)
    check(f"{tag} stats", stats, sv, sb)
    B, S, Q, _ = stats.shape
    g = torch.Generator().manual_seed(11)
    gamma = R.f32r((1 + 0.5 * torch.randn(4 * Q, generator=g, dtype=F64)) * torch.where(torch.arange(4 * Q) % 3 == 1, -1.0, 1.0))
    beta = R.f32r(0.3 * torch.randn(4 * Q, generator=g, dtype=F64))
    ab, mr = run_finalize(stats, None, gamma, beta, hw)
    k = R.gn_finalize(stats, None, gamma, beta, R.GN_EPS, hw)
    check(f"{tag} finalize-ab", ab, *k["ab"])
    check(f"{tag} finalize-mr", mr, *k["mr"])


def run_finalize(st1, st2, gamma, beta, hw):
    B, S1, Q1, _ = st1.shape
    C1, C2 = 4 * Q1, (4 * st2.shape[2] if st2 is not None else 0)
    G, _ = R.gn_geometry(C1 + C2)
    a1, a2, gm, bt = guarded(st1, torch.float32), guarded(st2, torch.float32), f32(gamma), f32(beta)
    runs = []
    for _ in range(2):
        ab, mr = nans((B, C1 + C2, 2)), nans((B, G, 2))
        call(_lib.lib().fg_op_edm_gn_finalize(ptr(a1), C1, S1, ptr(a2), C2, st2.shape[1] if st2 is not None else 0, ptr(gm), ptr(bt), R.GN_EPS, ptr(ab), ptr(mr), B,
                                              hw, None))
        runs.append((ab, mr))
    assert same_bits(runs[0][0], runs[1][0]) and same_bits(runs[0][1], runs[1][1]), "gn_finalize: two launches differ"
    return back(runs[0][0]), back(runs[0][1])


CONV_PARAMS = [(n, m, ws) for n in R.CONV_CASES for m in R.conv_modes(n)
               for ws in ((True, False) if R.expected_plan(m, R.CONV_CASES[n])[0] != R.K_GENERIC and not n.startswith(("sub_", "rs_")) else
                          ((True,) if n.startswith(("sub_", "rs_")) else (False,)))]


@pytest.mark.parametrize("name,mode,ws", CONV_PARAMS, ids=[f"{n}-{R.MODE_NAME[m]}-{'ws' if w else 'generic'}" for n, m, w in CONV_PARAMS])
def test_conv(name, mode, ws):
    d, ref = conv_ref(name, mode)
    outs, stats, plan = run_conv(d, mode, ws)
    want = R.expected_plan(mode, R.CONV_CASES[name]) if ws else (R.K_GENERIC, {32: 8, 16: 2, 8: 1}[d["h"]])
    assert plan == want, f"{name}: the dispatch takes {R.KERNEL_NAME.get(plan[0])} with {plan[1]} slots, expected {R.KERNEL_NAME[want[0]]} with {want[1]}"
    tag = f"conv {R.MODE_NAME[mode]} {name}-{R.KERNEL_NAME[plan[0]]}"
    for key, (v, b) in ref.items():
        check(f"{tag} {key}", outs[key], v, b)
    if stats is not None:
        check_stats_and_finalize(tag, outs["out"], stats, R.stats_layout(plan[0], d["res"]), d["h"] * d["h"])


@pytest.mark.parametrize("mode", [1, 2], ids=MODE_IDS)
@pytest.mark.parametrize("wrap", list(R.WRAP_CASES))
def test_conv_wrap(wrap, mode):
    """More tiles than CUs: a persistent workgroup walks on to a second tile.  The images are the base case's, cycled, so the base case's
    fp64 reference serves every image, per element."""
    name, batch = R.WRAP_CASES[wrap]
    base, ref = conv_ref(name, mode)
    d, idx = R.cycle_images(base, batch)
    kernel, slots = conv_plan(d, mode, True)
    assert kernel == (R.K_WS if mode == 1 else R.K_X3WS)
    tiles = batch * {32: 8, 16: 2}[d["h"]]  # 8 x 16 pixel tiles in both kernels (conv_ws.hip, conv_ws3.hip); slots = tiles (x 4 producer waves)
    assert slots == {32: 8, 16: 2}[d["h"]] * (1 if mode == 1 else 4)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert tiles > cus, f"{tiles} tiles do not wrap on {cus} CUs"
    outs, stats, plan = run_conv(d, mode, True)
    tag = f"conv {R.MODE_NAME[mode]} {wrap}-{R.KERNEL_NAME[kernel]}"
    v, b = ref["out"]
    check(f"{tag} out", outs["out"], v[idx], b[idx])
    sv, sb = R.slot_stats(outs["out"], R.stats_layout(kernel, d["res"]))
    check(f"{tag} stats", stats, sv, sb)


# ---- the statistics chain --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("offset", R.GN_OFFSETS)
@pytest.mark.parametrize("case", R.GN_SYNTH, ids=lambda c: "-".join(map(str, c)))
def test_gn_finalize_synthetic(case, offset):
    d = R.gn_synth_inputs(case, offset)
    ab, mr = run_finalize(d["st1"], d["st2"], d["gamma"], d["beta"], d["hw"])
    k = R.gn_finalize(d["st1"], d["st2"], d["gamma"], d["beta"], R.GN_EPS, d["hw"])
    tag = f"gn_finalize fp32 {'-'.join(map(str, case))}-off{offset}"
    check(f"{tag} ab", ab, *k["ab"])
    check(f"{tag} mr", mr, *k["mr"])


@functools.lru_cache(maxsize=None)
def conv_ref_acc(mode):
    d = R.conv_inputs(R.OFFSET_BASE, mode)
    return (d,) + R.conv_acc(d, mode)


@pytest.mark.parametrize("offset", R.GN_OFFSETS)
@pytest.mark.parametrize("mode", R.MODES, ids=MODE_IDS)
def test_mean_offset_chain(mode, offset):
    """conv -> slots -> gn_finalize on a tensor whose per-group mean / std is `offset`, judged by the derived bound, which carries the
    slots' fp32 error through the cancellation of sum v^2 / cnt - mean^2 and so grows with the offset (not capped).  The measured error
    of the normalised value, against the two-pass fp64 GroupNorm of the stored tensor, is printed.  Measured on an MI355X (32x32, 8
    channels per group, 128-pixel slots), at one std from the group mean | over every element of the heavy-tailed designed input:
        mean / std   fp32               bf16               bf16x3             worst err / bound
        0            1.9e-7 | 4.2e-6    1.9e-7 | 4.7e-6    1.9e-7 | 3.1e-6    0.21
        1            3.2e-7 | 2.4e-6    4.0e-7 | 5.1e-6    3.1e-7 | 3.5e-6    0.087
        4            1.4e-6 | 1.8e-5    8.8e-7 | 1.1e-5    1.3e-6 | 1.2e-5    0.017
        16           2.3e-5 | 3.9e-4    8.7e-6 | 1.4e-4    1.1e-5 | 1.4e-4    0.013
        64           3.3e-4 | 4.2e-3    1.0e-4 | 1.6e-3    2.2e-4 | 2.9e-3    0.012
    The error grows with the square of the offset and crosses the bf16x3 forward tolerance (2e-5) at mean / std of about 21 (bf16x3)
    and 15 (fp32) at one std from the mean, about 5 for the worst element (interpolated on the square law)."""
    d, acc, dacc, gamma, beta = R.offset_case(mode, offset, conv_ref_acc(mode))
    outs, stats, (kernel, slots) = run_conv(d, mode, R.expected_plan(mode, R.CONV_CASES[R.OFFSET_BASE])[0] != R.K_GENERIC)
    tag = f"offset {R.MODE_NAME[mode]} off{offset}-{R.KERNEL_NAME[kernel]}"
    check(f"{tag} out", outs["out"], *R.conv_epilogue(acc, dacc, d, mode)["out"])
    sv, sb = R.slot_stats(outs["out"], R.stats_layout(kernel, d["res"]))
    check(f"{tag} stats", stats, sv, sb)
    ab, _ = run_finalize(stats, None, gamma, beta, 1024)
    k = R.gn_finalize(sv, None, gamma, beta, R.GN_EPS, 1024, dst1=sb)
    e = lambda t: t[:, None, None, :]
    err = ((e(ab[..., 0]) - e(k["a"])) * outs["out"] + e(ab[..., 1]) - e(k["b"])).abs()
    bound = R.normalised_bound(outs["out"], k)
    # ... and at one standard deviation from the group's mean, where the unit-variance bulk of a normalised tensor lies
    ex = R.gn_coeffs_exact(outs["out"], gamma, beta, R.GN_EPS)
    da, db = ab[..., 0] - ex["a"], ab[..., 1] - ex["b"]
    unit = (da.abs() * ex["std"].repeat_interleave(8, 1) + (db + da * ex["mean"].repeat_interleave(8, 1)).abs()).max().item()
    print(f"OFFSET {R.MODE_NAME[mode]} {offset} at-1-sigma {unit:.3e} worst-element {err.max().item():.3e} bound {bound.max().item():.3e} "
          f"ratio {(err / bound).max().item():.4f}")
    assert (err <= bound).all(), (offset, (err / bound).max().item())


# ---- pool, stem, head -----------------------------------------------------------------------------------------------------------------------

def head_inputs(mode, B, res=32, C=128, cout=3):
    g = torch.Generator().manual_seed(7000 + B + mode)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    ts = [0.002, 80.0, 1.0][:B]  # coefficients at both ends of the noise range
    return dict(x_t=R.f32r(rn(B, cout, res, res) * torch.tensor(ts, dtype=F64)[:, None, None, None]), coef=R.edm_coef(ts),
                w_stem=R.f32r(rn(128, cout, 3, 3) / 27 ** 0.5), b_stem=R.f32r(rn(128)),
                x=R.to_storage(R.bordered(rn(B, res, res, C)), mode), ab=R.design_ab(B, C, g),
                w_aux=R.f32r(rn(cout, C, 3, 3) / (9 * C) ** 0.5), b_aux=R.f32r(rn(cout)))


def twice(fn, *outs_shape_dtype):
    runs = []
    for _ in range(2):
        outs = [nans(s, t) for s, t in outs_shape_dtype]
        fn(*outs)
        runs.append(outs)
    for a, b in zip(*runs):
        assert same_bits(a, b), "two launches differ"
    return [back(o) for o in runs[0]]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("mode", R.MODES, ids=MODE_IDS)
def test_pool_stem_head(mode, B):
    L = _lib.lib()
    h = head_inputs(mode, B)
    T, name = tdt(mode), R.MODE_NAME[mode]
    res, C, cout = 32, 128, 3
    x, ab, x_t, coef = guarded(h["x"], T), guarded(h["ab"], torch.float32), guarded(h["x_t"], torch.float32), f32(h["coef"])
    (got,) = twice(lambda o: call(L.fg_op_edm_gn_silu_pool(mode, ptr(x), ptr(ab), ptr(o), B, res // 2, C, None)), ((B, res // 2, res // 2, C), T))
    check(f"gn_silu_pool {name} b{B} out", got, *R.gn_silu_pool(h["x"], h["ab"], mode))
    ws, bs, wa, ba = f32(h["w_stem"]), f32(h["b_stem"]), f32(h["w_aux"]), f32(h["b_aux"])
    packed = torch.empty(max(L.fg_op_edm_head_pack_bytes(0, mode, 0), L.fg_op_edm_head_pack_bytes(1, mode, C)), dtype=torch.uint8, device=dev())
    got, st = twice(lambda o, s: call(L.fg_op_edm_stem(mode, ptr(x_t), ptr(coef), ptr(ws), ptr(packed), ptr(bs), ptr(o), ptr(s), B, res, cout, None)),
                    ((B, res, res, 128), T), ((B, res * res // 32, 32, 2), torch.float32))
    check(f"stem {name} b{B} out", got, *R.stem(h["x_t"], h["coef"][:B], h["w_stem"], h["b_stem"], mode, True))
    check_stats_and_finalize(f"stem {name} b{B}", got, st, "rows32", res * res)
    (got,) = twice(lambda o: call(L.fg_op_edm_conv_in(mode, ptr(x_t), ptr(coef), ptr(ws), ptr(bs), ptr(o), B, res, cout, 128, None)), ((B, res, res, 128), T))
    check(f"conv_in {name} b{B} out", got, *R.stem(h["x_t"], h["coef"][:B], h["w_stem"], h["b_stem"], mode, False))
    (got,) = twice(lambda o: call(L.fg_op_edm_aux_head(mode, ptr(x), ptr(ab), ptr(wa), ptr(packed), ptr(ba), ptr(x_t), ptr(coef), ptr(o), B, C, cout, None)),
                   ((B, cout, res, res), torch.float32))
    check(f"aux_head {name} b{B} out", got, *R.aux(h["x"], h["ab"], h["w_aux"], h["b_aux"], h["x_t"], h["coef"], mode, True))
    (got,) = twice(lambda o: call(L.fg_op_edm_aux_out(mode, ptr(x), ptr(ab), ptr(wa), ptr(ba), ptr(x_t), ptr(coef), ptr(o), B, res, C, cout, None)),
                   ((B, cout, res, res), torch.float32))
    check(f"aux_out {name} b{B} out", got, *R.aux(h["x"], h["ab"], h["w_aux"], h["b_aux"], h["x_t"], h["coef"], mode, False))


# ---- attention --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", R.MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", R.ATTN_CASES, ids=lambda c: "-".join(map(str, c)))
def test_attention(case, mode):
    T_, B, fam = case
    d = R.attn_inputs(case, mode)
    T = tdt(mode)
    q, k, vt = guarded(d["q"], T), guarded(d["k"], T), guarded(d["vt"], T)
    (got,) = twice(lambda o: call(_lib.lib().fg_op_edm_attention(mode, ptr(q), ptr(k), ptr(vt), ptr(o), B, T_, None)), ((B, T_, 256), T))
    check(f"attention {R.MODE_NAME[mode]} {T_}-{B}-{fam} out", got, *R.attention(d["q"], d["k"], d["vt"], mode))


@pytest.mark.parametrize("B", [1, 3])
def test_attention_merged(B):
    """The merged block from its three launches - attn_merge_weights, the OUT_QV 1x1 conv, the merged attention - each fed by the
    device's own output of the one before and judged against the reference of that stage; then the statistics and gn_finalize."""
    L = _lib.lib()
    m = R.merged_inputs(B)
    C = 256
    qkv_w, qkv_b, proj_w = f32(m["qkv_w"]), f32(m["qkv_b"]), f32(m["proj_w"])
    w, b = twice(lambda wo, bo: call(L.fg_op_edm_attn_merge_weights(ptr(qkv_w), ptr(qkv_b), ptr(proj_w), ptr(wo), ptr(bo), C, None)),
                 ((2 * C, C), torch.float32), ((2 * C,), torch.float32))
    (wv, wb), (bv, bb) = R.attn_merge_weights(m["qkv_w"], m["qkv_b"], m["proj_w"])
    check(f"attn_merge_weights fp32 b{B} w", w, wv, wb)
    check(f"attn_merge_weights fp32 b{B} b", b, bv, bb)
    d = dict(name=f"merged_qv_b{B}", ks=1, pro=R.PRO_GN, res=R.RES_NONE, outmode=R.OUT_QV, c1=C, c2=0, h=16, hs=16, B=B, cout=2 * C, qkv_perm=False, rshift=0,
             src1=m["x_mid"].reshape(B, 16, 16, C), src2=None, ab=m["ab"], w=w[:, :, None, None], bias=b, temb=None, resid=None, scale=1.0)
    outs, _, plan = run_conv(d, 2, False)
    assert plan[0] == R.K_GENERIC
    ref = R.conv(d, 2)
    check(f"conv bf16x3 merged_qv_b{B} q", outs["q"], *ref["q"])
    check(f"conv bf16x3 merged_qv_b{B} vt", outs["vt"], *ref["vt"])
    qm, vmt, x_mid, ab, bp = (guarded(t, torch.float32) for t in (outs["q"], outs["vt"], m["x_mid"], m["ab"], m["proj_b"]))
    got, st = twice(lambda o, s: call(L.fg_op_edm_attention_merged(ptr(qm), ptr(x_mid), ptr(ab), ptr(vmt), ptr(bp), R.SQRT_HALF, ptr(o), ptr(s), B, None)),
                    ((B, 256, C), torch.float32), ((B, 8, C // 4, 2), torch.float32))
    check(f"attention_merged bf16x3 b{B} out", got, *R.attention_merged(outs["q"], m["x_mid"], m["ab"], outs["vt"], m["proj_b"], R.SQRT_HALF))
    check_stats_and_finalize(f"attention_merged bf16x3 b{B}", got.reshape(B, 16, 16, C), st, "rows32", 256)


# ---- in situ: the ops are what the engine runs ------------------------------------------------------------------------------------------------

IN_SITU_TOL = {0: 1e-4, 1: (2 * 9) ** 0.5 * 2.0 ** -9, 2: 1e-4}


@pytest.mark.parametrize("mode", R.MODES, ids=MODE_IDS)
def test_in_situ_encoder_tap(mode):
    """fg_edm_forward_features' first tap (the 32x32 `block3` output of the encoder) at B = 3 against the same nine launches rebuilt from
    the op-level entry points: stem -> 4 x (gn_finalize -> conv0 + temb -> gn_finalize -> [1x1 skip] -> conv1 + residual), every
    GroupNorm fed by the statistics slots of the producer before it, the kernels those the plan names.  The one input the chain does
    not take from the device is temb = affine(emb): the embedding MLP is evaluated here in fp32 / fp64, a few fp32 ulps (about 1e-6
    relative) from the engine's own, which each block passes on with a gain of order 1 - so the two taps agree to rel-L2 1e-4 in the
    fp32-storage modes (measured 1.3e-6 fp32, 4.3e-6 bf16x3).  In bf16 the perturbation flips roundings, every flip (2^-8 of the
    element) perturbs the 9 x 256 outputs it feeds by more than their distance to a tie, and after a few stores the two chains round
    independently: each of the nine stored tensors (stem, 4 x (h, x)) then adds at most sqrt(2) 2^-9 in rel-L2, in quadrature
    sqrt(2 * 9) 2^-9 = 8.3e-3 (measured 4.5e-3).  A wrong op argument (eps, scale, slot count, residual, temb row) is 1e-2 or more in
    every mode; the per-element statement in bf16 is the per-op tests' above."""
    from fastgen_amd.networks.EDM.network import EDMPrecond
    from oracle import edm_ref as O

    L = _lib.lib()
    cfg, B, res = O.CIFAR10, 3, 32
    sd = O.random_state_dict(cfg, seed=4321)
    net = EDMPrecond(img_resolution=32, img_channels=3, label_dim=10, sigma_shift=0.0, sigma_data=0.5, model_type="SongUNet", augment_dim=9,
                     model_channels=128, channel_mult=[2, 2, 2], channel_mult_noise=1, embedding_type="positional", encoder_type="standard",
                     decoder_type="standard", resample_filter=[1, 1], dropout=0.0, label_dropout=0, r_timestep=False, drop_precond=None)
    net.load_state_dict(sd, strict=True)
    net = net.to(dev()).eval()
    net.compute_dtype = R.MODE_NAME[mode]
    g = torch.Generator().manual_seed(9)
    t = torch.tensor([0.5, 2.0, 40.0], dtype=F64)
    x_t = (torch.randn(B, 3, res, res, generator=g) * t[:, None, None, None].float()).contiguous()
    cond = torch.nn.functional.one_hot(torch.arange(B) % 10, 10).float()
    with torch.no_grad():  # the inference entry point (fg_edm_forward_features), not the kept forward of a training call
        (tap,) = net.forward(x_t.to(dev()), t.to(dev()), condition=cond.to(dev()), return_features_early=True, feature_indices={0})
    tap = back(tap)

    coef = R.edm_coef(t)
    emb = O.mapping(sd, cfg, coef[B:2 * B].float(), cond).to(F64)
    P = lambda name: sd[name].to(F64)
    T = tdt(mode)
    xd, coefd = f32(x_t.to(F64)), f32(coef)
    packed = torch.empty(L.fg_op_edm_head_pack_bytes(0, mode, 0), dtype=torch.uint8, device=dev())
    x, xst = nans((B, res, res, 128), T), nans((B, res * res // 32, 32, 2))
    ws_, bs_ = f32(P("model.enc.32x32_conv.weight")), f32(P("model.enc.32x32_conv.bias"))
    call(L.fg_op_edm_stem(mode, ptr(xd), ptr(coefd), ptr(ws_), ptr(packed), ptr(bs_), ptr(x), ptr(xst), B, res, 3, None))
    xslots, cin = res * res // 32, 128

    def finalize(st, c, slots, key):
        ab, gm, bt = nans((B, c, 2)), f32(P(f"{key}.weight")), f32(P(f"{key}.bias"))
        call(L.fg_op_edm_gn_finalize(ptr(st), c, slots, None, 0, 0, ptr(gm), ptr(bt), R.GN_EPS, ptr(ab), None, B, res * res, None))
        return ab

    def conv3(src, c, ab, key, temb, resid, scale):
        d = dict(ks=3, pro=R.PRO_GN_SILU, res=R.RES_NONE, outmode=R.OUT_NHWC, c1=c, c2=0, B=B, hs=res, h=res, cout=256, rshift=0)
        ws = R.expected_plan(mode, (3, R.PRO_GN_SILU, R.RES_NONE, R.OUT_NHWC, c, 0, res, B, ""))[0] != R.K_GENERIC
        kernel, slots = conv_plan(d, mode, ws)
        assert kernel == R.expected_plan(mode, (3, R.PRO_GN_SILU, R.RES_NONE, R.OUT_NHWC, c, 0, res, B, ""))[0]
        w = P(f"{key}.weight")
        wp = pack(w, mode, _lib.FG_EDM_PACK_GENERIC, 3)
        wws = pack(w, mode, _lib.FG_EDM_PACK_WS if mode == 1 else _lib.FG_EDM_PACK_X3WS, 3) if ws else None
        out, st, bias = nans((B, res, res, 256), T), nans((B, slots, 64, 2)), f32(P(f"{key}.bias"))
        call(L.fg_op_edm_conv(mode, 3, R.PRO_GN_SILU, R.RES_NONE, R.OUT_NHWC, ptr(src), c, None, 0, B, res, res, ptr(ab), ptr(wp), ptr(wws), ptr(bias), ptr(temb),
                              256 if temb is not None else 0, ptr(resid), 0, scale, ptr(out), 256, ptr(st), None, None, None, None))
        return out, st, slots

    for idx in range(4):
        key = f"model.enc.32x32_block{idx}"
        temb = f32(emb @ P(f"{key}.affine.weight").t() + P(f"{key}.affine.bias"))
        h, hst, hslots = conv3(x, cin, finalize(xst, cin, xslots, f"{key}.norm0"), f"{key}.conv0", temb, None, 1.0)
        resid = x
        if f"{key}.skip.weight" in sd:
            wsk, bsk, resid = pack(P(f"{key}.skip.weight"), mode, _lib.FG_EDM_PACK_GENERIC, 1), f32(P(f"{key}.skip.bias")), nans((B, res, res, 256), T)
            call(L.fg_op_edm_conv(mode, 1, R.PRO_NONE, R.RES_NONE, R.OUT_NHWC, ptr(x), cin, None, 0, B, res, res, None, ptr(wsk), None, ptr(bsk), None, 0, None, 0, 1.0,
                                  ptr(resid), 256, None, None, None, None, None))
        x, xst, xslots = conv3(h, 256, finalize(hst, 256, hslots, f"{key}.norm1"), f"{key}.conv1", None, resid, R.SQRT_HALF)
        cin = 256
    got = back(x).permute(0, 3, 1, 2)
    assert torch.isfinite(got).all() and torch.isfinite(tap).all()
    rel = ((got - tap).norm() / tap.norm()).item()
    print(f"IN-SITU {R.MODE_NAME[mode]} rel-L2 {rel:.3e} max|diff| {(got - tap).abs().max().item():.3e} max|tap| {tap.abs().max().item():.3e}")
    assert rel <= IN_SITU_TOL[mode], rel
