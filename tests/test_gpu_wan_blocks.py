"""Per-block and per-op parity of the causal video DiT (fastgen_amd/csrc/wan.hip, engine_wan.inc, the token GEMMs of gemm.hip, dit.hip's
LayerNorm-modulate) against the oracle's pieces (oracle/wan_ref.py) in fp64, per (sample, frame), per (sample, head) and per ragged
query tile, on every path the engine takes: inner widths 256 / 384 / 1536 / 2048 / 5120, batches that straddle the groups of 8 of the
sample-major attention mapping (with and without >= 1024 keys), chunk 0 without a cache, its store_kv = 1 call, chunk 1 over the cache, a
chunk on the RoPE table's clamp, the block-causal call with a frame remainder, frames of 15 and 96 tokens (no multiple of a GEMM or
query tile), 37 text tokens, fa2_kernel's uneven split and fa_kernel's key split, 8 latent channels in and out.

`fg_wan_forward_features` with every block tapped hands back, as fp32, the bf16 buffers the next kernel consumed.  Every sample has its
own x and text, every FRAME its own t in [0.05, 0.95].  Block i is run by the oracle on the GPU's own block input (the previous tap; block
0: tokens_out) and the GPU's temb_out; over a cache the test keeps its own fp64 K / V per block, computed by `self_attn_qkv` from the
GPU's block input at the store_kv = 1 call.  Compared are the INCREMENTS x_attn1 - x_in, x_attn2 - x_attn1, x_ffn - x_attn2 (the residual
stream would hide a wrong branch) and the pre-projection attention outputs; tokens_out, temb_out and the final output (on the GPU's last
stream) on their own.  At B >= 9 samples {0, 1, 7, 8, B - 1} are fetched and checked, otherwise all; always all frames.

Bounds: TOL, twice the worst value measured on an MI355X over the matrix.  tokens_out is the exception: the patch embedding computes in
fp32 and STORES bf16 (the stream's format), so it cannot land at 1e-5; it is held element by element to what the formats give,
|err| <= 2^-8 |ref| (half a bf16 ulp) + 2e-5 max |ref| (the fp32 dot product).

That the check sees is asserted, per call and block, with references mutated in fp64 from the oracle alone - each must miss the bound
5 times over: (a) the neighbouring sample's increments, (b) modulation rows (gate, MLP scale / shift) shifted by one frame, (c) RoPE
start_frame off by one (calls over a cache: RoPE is relative, without cached keys a common shift is the same function), (d) two heads
swapped in attn1, (e) the last 17 keys dropped, (f) the text K / V of the neighbouring sample, (g) cache_start off by one frame.

The tapped call changes nothing: its `out` is torch.equal to fg_wan_forward's (fg_wan_forward_block_causal's) on the same inputs and cache
state, and a second tapped call reports the same x_ffn.

The machinery below also serves tests/test_gpu_wan_full_blocks.py, the same pin of the bidirectional call: a call of kind "full"
(`fg_wan_forward_full` / `fg_wan_forward_full_features`) is ("full", 0, frames, 0, with_r, skip_layers) - no cache, no mask, start frame
0, every frame its own r beside its own t - and brings its own checks and mutants (m) - (q); that file describes them."""
import ctypes
import dataclasses
from dataclasses import dataclass

import pytest
import torch

from fastgen_amd import _lib
from oracle import wan_ref as R

pytestmark = pytest.mark.gpu

# (kind, cur_start_frame, frames, store_kv).  7 frames of capacity, chunks of 2 (block-causal: 3 | 2 | 2), a RoPE table of 5 rows:
# chunk 0 without a cache, its cache-fill call, chunk 1 over the cache, its cache-fill call, frames 4-6 (5 and 6 on the clamp), all frames
STD = (("ar", 0, 2, 0), ("ar", 0, 2, 1), ("ar", 2, 2, 0), ("ar", 2, 2, 1), ("ar", 4, 3, 0), ("bc", 0, 7, 0))


@dataclass
class Case:
    heads: int = 2
    ffn: int = 512
    B: int = 1
    lat: tuple = (10, 6)   # latent height x width: 5 x 3 = 15 tokens per frame
    text_len: int = 37
    chans: int = 16
    total: int = 7
    chunk: int = 2
    rope_max: int = 5
    calls: tuple = STD
    seed: int = 0
    # what only the bidirectional matrix sets (tests/test_gpu_wan_full_blocks.py)
    layers: int = 2
    r: str = ""             # "diff" / "abs": a `Wan` handle with a full-scale r_embedder of that time_cond_type (fg_wan_create_ex)
    dtype: str = ""         # "fp8": only the tapped call's `out` is compared, with the untapped call's
    device_oracle: bool = False  # the oracle's pieces run in fp64 on the GPU (thousands of tokens)


CASES = {
    # widths (B = 1)
    "D256": Case(seed=4), "D384": Case(heads=3, ffn=1024), "D1536": Case(heads=12, ffn=8960), "D2048": Case(heads=16, ffn=8192),
    "D5120": Case(heads=40, ffn=13824, calls=(("ar", 0, 2, 1), ("ar", 2, 3, 0))),  # (the oracle reads 4.8 GB of fp64 weights per call)
    # batch: B >= 8 runs fa_kernel<128> sample-major (L <= 1024, one key split); 9 and 11 straddle the groups of 8
    "B2": Case(B=2), "B3": Case(B=3), "B8": Case(B=8), "B9": Case(B=9), "B11": Case(B=11),
    "D1536-B8": Case(heads=12, ffn=8960, B=8),
    # sample-major over >= 1024 keys (where it displaces fa2_kernel): 96-token frames, 10 cached frames, 10 more (960 queries, 1920 keys)
    "B9-keys1920": Case(B=9, lat=(16, 24), total=20, rope_max=16, calls=(("ar", 0, 10, 1), ("ar", 10, 10, 0))),
    # 96-token frames, B = 2: 576 and 864 keys (fa_kernel, key-split by the cost model), 1152 keys (fa2_kernel, uneven split)
    "B2-fs96": Case(B=2, lat=(16, 24), total=12, chunk=3, rope_max=16,
                    calls=(("ar", 0, 6, 1), ("ar", 6, 3, 0), ("ar", 6, 3, 1), ("ar", 9, 3, 0))),
    # generic patch-embed kernel, C != 16 in the final kernel
    "C8": Case(B=2, chans=8),
}

# (relative L2, max |err| / max |ref|) per granule = twice the worst measured on an MI355X over the matrix: temb 1.09e-5 / 1.35e-5;
# attn1 per (sample, frame | head | last tile) 1.20e-2 / 2.88e-2, per (sample, query, head) 4.37e-2 / 4.73e-2; inc1 2.19e-2 / 2.22e-2;
# attn2 5.10e-3 / 1.15e-2, per query 1.04e-2 / 1.33e-2; inc2 8.65e-3 / 1.84e-2; ffn 1.73e-2 / 2.21e-2; out 1.92e-7 / 2.63e-7;
# tokens_out 0.985 of its derived bound.  (The increments are differences of two bf16-stored streams: their error is the stream's
# rounding, 2^-9 of |x|, over the increment's size - larger than the attention outputs', which are stored once.)
# Smallest distance of a mutant from the GPU, relative L2 in the granule named in run_case: (a) 1.05 / 0.53 / 1.09 (inc1 / inc2 / ffn),
# (b) 1.02 / 1.06, (d) 1.37, (e) 0.88, (f) 0.46 / 0.47, (g) 1.44 - 10 to 57 times their bounds; (c), per (sample, frame | head), 6 to 8 times its bound (a one-frame RoPE shift turns only the
# lowest few of the 22 temporal pairs noticeably: the weakest of the mutants, and the reason for Q_GAIN and for D256's seed).
TOL = {
    "temb": (2.2e-5, 2.7e-5), "attn1": (2.4e-2, 5.8e-2), "attn1/row": (8.8e-2, 9.5e-2), "inc1": (4.4e-2, 4.5e-2),
    "attn2": (1.05e-2, 2.3e-2), "attn2/row": (2.1e-2, 2.7e-2), "inc2": (1.75e-2, 3.7e-2), "ffn": (3.5e-2, 4.5e-2), "out": (4e-7, 5.5e-7),
}
TOK_ULP, TOK_ABS = 2.0 ** -8, 2e-5  # tokens_out: half a bf16 ulp of the stored value + the fp32 dot product
MUTANT_FACTOR = 5.0
Q_GAIN = 3.0


def _checked(B):
    return list(range(B)) if B < 9 else sorted({0, 1, 7, 8, B - 1})


def _cfg(c: Case) -> R.WanConfig:
    return R.WanConfig(num_heads=c.heads, head_dim=128, in_channels=c.chans, out_channels=c.chans, text_dim=64, ffn_dim=c.ffn, num_layers=c.layers,
                       rope_max_seq_len=c.rope_max, chunk_size=c.chunk, total_num_frames=c.total)


def _inputs(c: Case, cfg, call, ci, seed):
    """x [B, C, F, H, W] and the embedder's per-frame timesteps [B, F] (fp32, 1000 t with t spread over [0.05, 0.95], no two alike);
    third, for a "full" call, the second embedder's rows r [B, F] (else None): t and r are 2 B F distinct points of the same grid,
    paired at random, the larger of a pair being t - no two of the 2 B F values coincide and t - r > 0 in every frame."""
    g = torch.Generator().manual_seed(1000 * seed + ci)
    Fr = call[2]
    x = torch.randn((c.B, c.chans, Fr) + tuple(c.lat), generator=g)
    n = c.B * Fr
    if call[0] == "full":
        v = (0.05 + 0.9 * (torch.randperm(2 * n, generator=g).double() + 0.5) / (2 * n)).view(n, 2)
        t, r = v.amax(1).view(c.B, Fr), v.amin(1).view(c.B, Fr)
        return x, (1000.0 * t).float(), (1000.0 * r).float()
    t = (0.05 + 0.9 * (torch.randperm(n, generator=g).double() + 0.5) / n).view(c.B, Fr)
    return x, (1000.0 * t).float(), None


class Gpu:
    """The engine behind the drop-in module, called through the C ABI directly."""

    def __init__(self, c: Case, cfg, sd):
        from fastgen_amd.networks.Wan.network import Wan
        from fastgen_amd.networks.Wan.network_causal import CausalWan

        self.dev = torch.device("cuda:0")
        kw = dict(num_attention_heads=cfg.num_heads, attention_head_dim=128, in_channels=cfg.in_channels, out_channels=cfg.out_channels,
                  text_dim=cfg.text_dim, ffn_dim=cfg.ffn_dim, num_layers=cfg.num_layers, rope_max_seq_len=cfg.rope_max_seq_len,
                  compute_dtype=c.dtype or None)
        if c.r:  # (the r_embedder is the bidirectional module's; its handle's chunk_size and total_num_frames are 1)
            net = Wan(r_timestep=True, time_cond_type=c.r, **kw)
        else:
            net = CausalWan(chunk_size=cfg.chunk_size, total_num_frames=cfg.total_num_frames, **kw)
        net.load_state_dict(sd, strict=True)
        self.net = net.to(self.dev).eval()
        self.net._bind(self.dev)
        self.cfg, self.B, self.lat = cfg, c.B, c.lat
        self.L = _lib.lib()
        self.stream = ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
        need = max([1] + [(self.L.fg_wan_full_workspace_bytes if k[0] == "full" else self.L.fg_wan_workspace_bytes)(
            self.net._h, c.B, k[2], c.lat[0], c.lat[1]) for k in c.calls])
        self.ws = torch.empty(need, dtype=torch.uint8, device=self.dev)

    def set_text(self, text):
        self.text = text.to(self.dev).contiguous()
        _lib.check(self.L.fg_wan_set_text(self.net._h, ctypes.c_void_p(self.text.data_ptr()), self.B, text.shape[1],
                                          ctypes.c_void_p(self.ws.data_ptr()), self.ws.numel(), self.stream))

    def _full_args(self, call, rf):
        """r_frames (device tensor or None) and skip_layers / num_skip of a "full" call."""
        self.rd = rf.to(self.dev).contiguous() if call[4] else None
        skip = tuple(call[5])
        return ctypes.c_void_p(self.rd.data_ptr()) if call[4] else None, (ctypes.c_int * len(skip))(*skip) if skip else None, len(skip)

    def plain(self, call, x, tf, rf=None):
        """fg_wan_forward / fg_wan_forward_block_causal / fg_wan_forward_full: out [B, C, F, H, W] on the device."""
        kind, start, Fr, store = call[:4]
        self.xd, self.td = x.to(self.dev).contiguous(), tf.to(self.dev).contiguous()
        out = torch.full_like(self.xd, float("nan"))
        p = lambda v: ctypes.c_void_p(v.data_ptr())  # noqa: E731
        if kind == "full":
            r_ptr, skip, nskip = self._full_args(call, rf)
            _lib.check(self.L.fg_wan_forward_full(self.net._h, p(self.xd), p(self.td), r_ptr, p(out), self.B, Fr, self.lat[0], self.lat[1], skip,
                                                  nskip, p(self.ws), self.ws.numel(), self.stream))
        elif kind == "bc":
            _lib.check(self.L.fg_wan_forward_block_causal(self.net._h, p(self.xd), p(self.td), p(out), self.B, Fr, self.lat[0], self.lat[1],
                                                          p(self.ws), self.ws.numel(), self.stream))
        else:
            _lib.check(self.L.fg_wan_forward(self.net._h, p(self.xd), p(self.td), p(out), self.B, Fr, self.lat[0], self.lat[1], start, store,
                                             p(self.ws), self.ws.numel(), self.stream))
        return out

    def tapped(self, call, x, tf, rf=None):
        """fg_wan_forward_features (fg_wan_forward_full_features) with everything tapped: dict of device tensors; a skipped block: None."""
        kind, start, Fr, store = call[:4]
        cfg, B = self.cfg, self.B
        Ltok, D, depth = Fr * (self.lat[0] // 2) * (self.lat[1] // 2), cfg.dim, cfg.num_layers
        self.xd, self.td = x.to(self.dev).contiguous(), tf.to(self.dev).contiguous()
        new = lambda *s: torch.full(s, float("nan"), device=self.dev)  # noqa: E731
        r = dict(out=torch.full_like(self.xd, float("nan")), tokens=new(B, Ltok, D), temb=new(B * Fr, D),
                 blocks=[{k: new(B, Ltok, D) for k in ("attn1", "x_attn1", "attn2", "x_attn2", "x_ffn")} for _ in range(depth)])
        p = lambda v: ctypes.c_void_p(v.data_ptr())  # noqa: E731
        if kind == "full":
            r_ptr, skip, nskip = self._full_args(call, rf)
            r["blocks"] = [None if i in call[5] else b for i, b in enumerate(r["blocks"])]
            r["tproj"] = new(B * Fr, 6 * D)
            live = [i for i in range(depth) if i not in call[5]]
            taps = (_lib.fg_wan_block_taps * len(live))()
            for j, i in enumerate(live):
                for k, v in r["blocks"][i].items():
                    setattr(taps[j], k, v.data_ptr())
            _lib.check(self.L.fg_wan_forward_full_features(self.net._h, p(self.xd), p(self.td), r_ptr, p(r["out"]), B, Fr, self.lat[0], self.lat[1],
                                                           skip, nskip, (ctypes.c_int * len(live))(*live), taps, len(live), p(r["tokens"]),
                                                           p(r["temb"]), p(r["tproj"]), p(self.ws), self.ws.numel(), self.stream))
            return r
        taps = (_lib.fg_wan_block_taps * depth)()
        for i, b in enumerate(r["blocks"]):
            for k, v in b.items():
                setattr(taps[i], k, v.data_ptr())
        _lib.check(self.L.fg_wan_forward_features(self.net._h, p(self.xd), p(self.td), p(r["out"]), B, Fr, self.lat[0], self.lat[1], start, store,
                                                  1 if kind == "bc" else 0, (ctypes.c_int * depth)(*range(depth)), taps, depth, p(r["tokens"]),
                                                  p(r["temb"]), p(self.ws), self.ws.numel(), self.stream))
        return r

    def close(self):
        del self.net, self.ws
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


def _fetch(r, rows, Fr, odev="cpu"):
    """The checked samples of a tapped call's results, fp64 where the oracle runs (the CPU, or the GPU for the largest cases)."""
    idx = torch.tensor(rows, device=r["out"].device)
    D = r["temb"].shape[1]
    get = lambda v: v[idx].double().to(odev)  # noqa: E731
    g = dict(out=get(r["out"]), tokens=get(r["tokens"]), temb=get(r["temb"].view(-1, Fr, D)).reshape(-1, D),
             blocks=[b and {k: get(v) for k, v in b.items()} for b in r["blocks"]])
    if "tproj" in r:
        g["tproj"] = get(r["tproj"].view(-1, Fr, 6 * D)).reshape(-1, 6 * D)
    return g


def _err(e, d, dims):
    """(relative L2, max |e| / max |d|) over `dims`, flattened over what is left (the granules)."""
    rel = e.pow(2).sum(dims).sqrt() / d.pow(2).sum(dims).sqrt()
    mx = e.abs().amax(dims) / d.abs().amax(dims)
    return rel.reshape(-1), mx.reshape(-1)


class Report:
    def __init__(self, tol):
        self.tol, self.worst, self.bad, self.mut = tol, {}, [], {}

    def check(self, what, where, got, ref, base, views):
        """got against ref, both minus base, at every granularity of `views`: [(label, reshape, dims reduced)]."""
        e, d = got - ref, ref - base
        for label, shape, dims in views:
            rel, mx = _err(e.reshape(shape), d.reshape(shape), dims)
            w = self.worst.get(what, (0.0, 0.0))
            self.worst[what] = (max(w[0], float(rel.max())), max(w[1], float(mx.max())))
            b = self.tol[what]
            for j in (~((rel <= b[0]) & (mx <= b[1]))).nonzero().flatten().tolist()[:16]:  # (NaN fails; 16 granules name the place)
                self.bad.append((what, where, label, j, float(rel[j]), float(mx[j])))

    def mutant(self, name, what, where, got, mref, base, views, every=False):
        """A mutated reference must miss the bound of `what` MUTANT_FACTOR times over: in the worst granule, or (every) in each."""
        e, d = got - mref, mref - base
        best = 0.0 if not every else float("inf")
        for label, shape, dims in views:
            rel, _ = _err(e.reshape(shape), d.reshape(shape), dims)
            rel = torch.nan_to_num(rel, nan=0.0)
            best = min(best, float(rel.min())) if every else max(best, float(rel.max()))
        ratio = best / self.tol[what][0]
        self.mut[name] = min(self.mut.get(name, float("inf")), ratio)
        if not ratio >= MUTANT_FACTOR:
            self.bad.append(("mutant not seen", name, what, where, ratio))


def _views(B, Fr, L, D, heads=None):
    """Granules of a [B, L, D] tensor: (sample, frame); for attention outputs also (sample, head) and the last (ragged) 128-row query tile."""
    v = [("sample,frame", (B, Fr, L // Fr, D), (2, 3))]
    if heads:
        v.append(("sample,head", (B, L, heads, D // heads), (1, 3)))
    return v


def _tile(x, L):
    return x[:, 128 * ((L - 1) // 128):]


def _rope_clamped(cfg, Fr, gh, gw, last):
    """Mutant (n): RoPE from frame 0 with the TEMPORAL rows of frame f taken at min(f, last) (the first t_dim columns of a row)."""
    t_dim = cfg.head_dim - 4 * (cfg.head_dim // 6)
    idx = torch.clamp(torch.arange(Fr), max=last)
    out = []
    for v in R.rope_for_chunk(cfg, Fr, gh, gw, 0, torch.float64):
        v = v.view(Fr, gh * gw, cfg.head_dim).clone()
        v[:, :, :t_dim] = v[idx][:, :, :t_dim]
        out.append(v.view(Fr * gh * gw, cfg.head_dim))
    return out


def _block(p, cfg, i, x, mod, cos, sin, kv2):
    """Block i of the oracle under full self-attention: the stream behind it (mutant (q) runs the blocks a call passes over)."""
    q, k, v = R.self_attn_qkv(p, cfg, i, x, mod, cos, sin)
    x1 = R.self_attn_out(p, i, x, R.sdpa(q, k, v), mod)
    return R.ffn(p, cfg, i, R.cross_attn(p, cfg, i, x1, *kv2)[1], mod)


def run_case(c: Case, make_gpu, tol=TOL):
    """One case of the matrix: every call of its sequence, every block, every check.  make_gpu(c, cfg, sd) -> Gpu."""
    cfg = _cfg(c)
    seed = 4000 + c.seed + 7 * c.heads + c.B
    if c.r:  # the same draws, and behind them a second embedder at the first one's scale
        import wan_full_ref

        sd = wan_full_ref.random_state_dict(cfg, seed=seed, r_timestep=True)
    else:
        sd = R.random_state_dict(cfg, seed=seed)
    for k in sd:  # sharper self-attention than the fan-in scaled draw gives (score spread ~ Q_GAIN): positions and single keys matter
        if k.endswith("attn1.norm_q.weight"):
            sd[k] = sd[k] * Q_GAIN
    gpu = make_gpu(c, cfg, sd)
    # pe: the weights on the CPU (the embedders and the patch embedding always run there); p: where the oracle's blocks run
    odev = torch.device("cuda:0" if c.device_oracle else "cpu")
    pe = {k[len("transformer."):]: v.double() for k, v in sd.items()}
    p = {k: v.to(odev) for k, v in pe.items()} if c.device_oracle else pe
    pr = {k.replace("r_embedder.", "condition_embedder."): v for k, v in pe.items() if k.startswith("r_embedder.")}
    del sd
    rows = _checked(c.B)
    Bc, D, H = len(rows), cfg.dim, cfg.num_heads
    gh, gw = c.lat[0] // 2, c.lat[1] // 2
    fs = gh * gw
    cap = cfg.total_num_frames * fs
    rep = Report(tol)
    text = torch.randn(c.B, c.text_len, cfg.text_dim, generator=torch.Generator().manual_seed(seed + 1))
    with torch.no_grad():
        gpu.set_text(text)
        ctx = R.text_embedding(p, text[rows].double().to(odev))
        kv2 = [R.cross_kv(p, cfg, i, ctx) for i in range(cfg.num_layers)]
        cached = any(k[0] == "ar" for k in c.calls)
        Kc = [torch.zeros(Bc, cap, H, 128, dtype=torch.float64) for _ in range(cfg.num_layers if cached else 0)]
        Vc = [torch.zeros(Bc, cap, H, 128, dtype=torch.float64) for _ in range(cfg.num_layers if cached else 0)]
        for ci, call in enumerate(c.calls):
            kind, start, Fr, store = call[:4]
            full = kind == "full"
            use_r, skipped = (bool(call[4]), tuple(call[5])) if full else (False, ())
            L, cs = Fr * fs, start * fs
            x, tf, rf = _inputs(c, cfg, call, ci, seed)
            # the untapped path is unchanged: same `out`, and a second tapped call reports the same taps
            out_plain = gpu.plain(call, x, tf, rf)
            r1 = gpu.tapped(call, x, tf, rf)
            r2 = gpu.tapped(call, x, tf, rf)
            if not torch.equal(out_plain, r1["out"]):
                rep.bad.append(("tapped out != fg_wan_forward's", ci))
            for i in range(cfg.num_layers):
                if i not in skipped and not torch.equal(r1["blocks"][i]["x_ffn"], r2["blocks"][i]["x_ffn"]):
                    rep.bad.append(("x_ffn tap differs between two calls", ci, i))
            if c.dtype == "fp8":  # (per-block bounds of that mode: not this matrix's)
                del out_plain, r1, r2
                continue
            g = _fetch(r1, rows, Fr, odev)
            del out_plain, r1, r2
            sf = _views(Bc, Fr, L, D)
            sfh = _views(Bc, Fr, L, D, H)
            tile = [("sample,last tile", (Bc, -1), (1,))]
            row = [("sample,query,head", (Bc, L, H, 128), (3,))]
            zero = torch.zeros((), dtype=torch.float64, device=odev)
            per_row = lambda n: [("sample,frame", (Bc * Fr, n), (1,))]  # noqa: E731
            # temb: fourier features and the embedder linears in fp32, on the timesteps the kernels read
            temb_ref = R.time_embedding(pe, cfg, tf[rows].double().reshape(-1))
            mut_tproj = {}
            if full:
                # ... and with r_frames the second embedder's rows on fp32(t - r) ("diff"; wan_r_rows_kernel) or r: temb + remb, and
                # timestep_proj + r_timestep_proj (the `tproj` tap: what every block's modulation is formed from)
                tproj_ref = R.time_projection(pe, temb_ref)
                if use_r:
                    def r_term(r_rows, diff):
                        remb = R.time_embedding(pr, cfg, ((tf[rows] - r_rows) if diff else r_rows).double().reshape(-1))
                        return remb, R.time_projection(pr, remb)

                    temb_t, tproj_t, diff = temb_ref, tproj_ref, c.r == "diff"
                    remb, rproj = r_term(rf[rows], diff)
                    temb_ref, tproj_ref = temb_t + remb, tproj_t + rproj
                    # (o) r taken per sample: every frame is given its neighbour's r.  (p) the wrong r term: none; the other
                    # time_cond_type; r_timestep_proj added but remb not (wan_full_ref.WanFullRef's mutants)
                    mo, mp = r_term(rf[rows].roll(1, 1), diff), r_term(rf[rows], not diff)
                    muts = {"o": (temb_t + mo[0], tproj_t + mo[1]), "p:ignore_r": (temb_t, tproj_t), "p:swap_cond": (temb_t + mp[0], tproj_t + mp[1]),
                            "p:proj_only": (temb_t, None)}
                    for name, (me_, mp_) in muts.items():
                        rep.mutant(name + ":temb", "temb", (ci,), g["temb"], me_.to(odev), zero, per_row(D), every=True)
                        if mp_ is not None:
                            rep.mutant(name + ":tproj", "tproj", (ci,), g["tproj"], mp_.to(odev), zero, per_row(6 * D), every=True)
                    mut_tproj = {k: muts[k][1].to(odev) for k in ("p:ignore_r", "p:swap_cond")}
                rep.check("tproj", (ci,), g["tproj"], tproj_ref.to(odev), zero, per_row(6 * D))
            rep.check("temb", (ci,), g["temb"], temb_ref.to(odev), zero, per_row(D))
            # tokens_out: fp32 patch embedding stored as bf16, element by element
            tok = R.patch_embed(pe, x[rows].double()).to(odev)
            q_ = ((g["tokens"] - tok).abs() / (TOK_ULP * tok.abs() + TOK_ABS * tok.abs().max())).max()
            rep.worst["tok/derived"] = (max(rep.worst.get("tok/derived", (0.0, 0.0))[0], float(q_)), 0.0)
            if not q_ <= 1.0:
                rep.bad.append(("tokens_out", ci, float(q_)))
            # the rows the blocks read: the GPU's own (the full call taps them; else they are one fp32 linear behind the temb tap)
            tproj = g["tproj"] if full else R.time_projection(p, g["temb"])
            cos, sin = (v.to(odev) for v in R.rope_for_chunk(cfg, Fr, gh, gw, start, torch.float64))
            mask = R.blockwise_causal_mask(Fr, fs, cfg.chunk_size) if kind == "bc" else None
            x_in = g["tokens"]
            pending = []  # the blocks the call passed over since the last one it ran
            for i, tap in enumerate(g["blocks"]):
                if tap is None:  # skipped: the next block's input is still x_in
                    pending.append(i)
                    continue
                w = (ci, i)
                mod = R.modulation(p, i, tproj, Bc, Fr)
                q, k, v = R.self_attn_qkv(p, cfg, i, x_in, mod, cos, sin)
                kf, vf = (k, v) if kind != "ar" else (torch.cat([Kc[i][:, :cs], k], 1), torch.cat([Vc[i][:, :cs], v], 1))
                att1 = R.sdpa(q, kf, vf, mask)
                x1 = R.self_attn_out(p, i, x_in, att1, mod)
                att2, x2 = R.cross_attn(p, cfg, i, x1, *kv2[i])
                x3 = R.ffn(p, cfg, i, x2, mod)
                g1, g2, g3 = tap["x_attn1"] - x_in, tap["x_attn2"] - tap["x_attn1"], tap["x_ffn"] - tap["x_attn2"]
                r1_, r2_, r3_ = x1 - x_in, x2 - x1, x3 - x2
                rep.check("attn1", w, tap["attn1"], att1, zero, sfh)
                rep.check("attn1", w, _tile(tap["attn1"], L), _tile(att1, L), zero, tile)
                rep.check("attn1/row", w, tap["attn1"], att1, zero, row)
                rep.check("inc1", w, g1, r1_, zero, sf)
                rep.check("attn2", w, tap["attn2"], att2, zero, sfh)
                rep.check("attn2", w, _tile(tap["attn2"], L), _tile(att2, L), zero, tile)
                rep.check("attn2/row", w, tap["attn2"], att2, zero, row)
                rep.check("inc2", w, g2, r2_, zero, sf)
                rep.check("ffn", w, g3, r3_, zero, sf)
                # ---- the mutants ----
                if Bc > 1:  # (a) the neighbouring sample's increments
                    for what, gg, rr in (("inc1", g1, r1_), ("inc2", g2, r2_), ("ffn", g3, r3_)):
                        rep.mutant("a:" + what, what, w, gg, rr.roll(1, 0), zero, sf, every=True)
                    # (f) the text K / V of the neighbouring sample
                    m2, mx2 = R.cross_attn(p, cfg, i, x1, kv2[i][0].roll(1, 0), kv2[i][1].roll(1, 0))
                    rep.mutant("f:attn2", "attn2", w, tap["attn2"], m2, zero, sfh, every=True)
                    rep.mutant("f:inc2", "inc2", w, g2, mx2 - x1, zero, sf, every=True)
                if Fr > 1:  # (b) modulation rows shifted by one frame: the gate of the attention residual, the MLP's scale / shift / gate
                    ms = mod.roll(1, 1)
                    rep.mutant("b:inc1", "inc1", w, g1, R.self_attn_out(p, i, x_in, att1, ms) - x_in, zero, sf)
                    rep.mutant("b:ffn", "ffn", w, g3, R.ffn(p, cfg, i, x2, ms) - x2, zero, sf)
                if cs > 0:  # (c) RoPE start_frame off by one (towards the table's inside), (g) cache_start off by one frame
                    s2 = start + 1 if start + Fr < cfg.rope_max_seq_len else start - 1
                    c2, n2 = R.rope_for_chunk(cfg, Fr, gh, gw, s2, torch.float64)
                    qm, km, _ = R.self_attn_qkv(p, cfg, i, x_in, mod, c2, n2)
                    mc = R.sdpa(qm, torch.cat([Kc[i][:, :cs], km], 1), vf)
                    rep.mutant("c:attn1", "attn1", w, tap["attn1"], mc, zero, sfh)
                    mg = R.sdpa(q, torch.cat([Kc[i][:, :cs - fs], k], 1), torch.cat([Vc[i][:, :cs - fs], v], 1))
                    rep.mutant("g:attn1", "attn1/row", w, tap["attn1"], mg, zero, row)
                hp = torch.arange(H)
                hp[0], hp[1] = 1, 0  # (d) two heads swapped
                rep.mutant("d:attn1", "attn1", w, tap["attn1"], att1.view(Bc, L, H, 128)[:, :, hp].reshape(Bc, L, D), zero, sfh)
                # (e) the last 17 keys dropped (block-causal: only the last chunk's queries see them)
                me = R.sdpa(q, kf[:, :-17], vf[:, :-17], None if mask is None else mask[:, :-17])
                rep.mutant("e:attn1", "attn1/row", w, tap["attn1"], me, zero, row)
                if full and Fr > cfg.chunk_size:  # (m) the block-causal mask of the config's chunk_size in place of full attention
                    mm = R.blockwise_causal_mask(Fr, fs, cfg.chunk_size).to(odev)
                    rep.mutant("m:attn1", "attn1", w, tap["attn1"], R.sdpa(q, k, v, mm), zero, sfh)
                    del mm
                if full and Fr > cfg.total_num_frames:  # (n) the temporal RoPE index clamped at total_num_frames - 1
                    c2, n2 = (t_.to(odev) for t_ in _rope_clamped(cfg, Fr, gh, gw, cfg.total_num_frames - 1))
                    qm, km, _ = R.self_attn_qkv(p, cfg, i, x_in, mod, c2, n2)
                    rep.mutant("n:attn1", "attn1", w, tap["attn1"], R.sdpa(qm, km, v), zero, sfh)
                for name, tp_m in mut_tproj.items():  # (p) again, through the rows the wrong r term hands the blocks
                    ms = R.modulation(p, i, tp_m, Bc, Fr)
                    rep.mutant(name + ":inc1", "inc1", w, g1, R.self_attn_out(p, i, x_in, att1, ms) - x_in, zero, sf)
                    rep.mutant(name + ":ffn", "ffn", w, g3, R.ffn(p, cfg, i, x2, ms) - x2, zero, sf)
                if pending:  # (q) skip ignored: the reference runs the blocks the call passed over, and this block behind them
                    xm = x_in
                    for j in pending:
                        xm = _block(p, cfg, j, xm, R.modulation(p, j, tproj, Bc, Fr), cos, sin, kv2[j])
                    qm, km, vm = R.self_attn_qkv(p, cfg, i, xm, mod, cos, sin)
                    rep.mutant("q:inc1", "inc1", w, g1, R.self_attn_out(p, i, xm, R.sdpa(qm, km, vm), mod) - x_in, zero, sf, every=True)
                    pending = []
                if kind == "ar" and store:
                    Kc[i][:, cs:cs + L], Vc[i][:, cs:cs + L] = k, v
                x_in = tap["x_ffn"]
            out_views = [("sample,frame", (Bc, cfg.out_channels, Fr, -1), (1, 3))]
            rep.check("out", (ci,), g["out"], R.final_layer(p, cfg, x_in, g["temb"], Fr, gh, gw), zero, out_views)
            if pending:  # (q) at the network's end: the output layer behind the blocks the call passed over
                xm = x_in
                for j in pending:
                    xm = _block(p, cfg, j, xm, R.modulation(p, j, tproj, Bc, Fr), cos, sin, kv2[j])
                rep.mutant("q:out", "out", (ci,), g["out"], R.final_layer(p, cfg, xm, g["temb"], Fr, gh, gw), zero, out_views, every=True)
            if use_r:  # (p) "proj only" changes temb alone, which the output layer's modulation reads
                rep.mutant("p:proj_only:out", "out", (ci,), g["out"], R.final_layer(p, cfg, x_in, temb_t.to(odev), Fr, gh, gw), zero, out_views,
                           every=True)
    gpu.close()
    return rep


@pytest.mark.parametrize("name", list(CASES))
def test_blocks(name):
    rep = run_case(CASES[name], Gpu)
    print(f"\n[wan-blocks] {name} " + " ".join(f"{k}={v[0]:.2e}/{v[1]:.2e}" for k, v in rep.worst.items()))
    print(f"[wan-blocks] {name} mutants (x bound) " + " ".join(f"{k}={v:.3g}" for k, v in rep.mut.items()))
    assert not rep.bad, rep.bad
