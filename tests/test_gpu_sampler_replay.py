"""The replay path of the five fused sampler loops (fg_sampler_run, fg_edm2_sampler_run, fg_dit_sampler_run, fg_wan_sampler_run,
fg_wan_guided_sampler_run).  Each loop is captured once as a hipGraph (the video loops: one per chunk) and replayed while the key of
`graph_run` matches; `fg_graph_stats` counts the graphs instantiated and launched, and the tests read its differences around a call.

Library level: the entry points through ctypes on buffers the test owns and reuses, so that every address in the key is stable by
construction.  The reference of every comparison is the same entry point with use_graph = 0 on the same values, and the agreement
asked is `torch.equal`: graph and eager launch the same kernels on the same buffers.
  a. a first call captures (one graph, two for the two chunks of the video loops), an identical second call captures nothing;
  b. nothing is baked in by value: other contents of the same buffers, other timesteps of the same zero pattern, another seed;
  c. what a graph must not be replayed for: every argument that a launch bakes in has to miss;
  d. one video call in which one chunk replays and the other is captured, on top of the cache bookkeeping a replay applies by hand;
  e. eager and graph calls, two shapes, and the two cache tags interleaved on one handle;
  f. weights updated in place between two graph calls.
Wrapper level: two calls of the public methods with equal values in freshly allocated tensors - the second has to replay.

Configurations: the smallest of the suite per family - the SongUNet of tests/test_gpu_parity.py (the only one the library builds for),
NARROW of the two ADM-style U-Nets, DiT tag "s" of tests/test_dit.py (and a two-block r_timestep DiT for the MeanFlow loop), the
causal video DiT of tests/test_wan.py at B=2, F=5, 16x24 (chunks of 3 + 2 frames); three steps."""
import ctypes

import pytest
import torch

import dhariwal_ref as ADM
import edm2_ref as E2
from fastgen_amd import _lib
from fastgen_amd.methods.model import FastGenModel
from fastgen_amd.networks.DiT.network import DiT
from fastgen_amd.networks.EDM.network import EDMPrecond
from fastgen_amd.networks.EDM2.network import EDM2Precond
from fastgen_amd.networks.Wan import solvers
from fastgen_amd.networks.Wan.network_causal import CausalWan
from oracle import dit_ref, edm_ref, wan_ref

pytestmark = pytest.mark.gpu

SONG = dict(img_resolution=32, img_channels=3, label_dim=10, sigma_shift=0.0, sigma_data=0.5, model_type="SongUNet", augment_dim=9,
            model_channels=128, channel_mult=[2, 2, 2], channel_mult_noise=1, embedding_type="positional", encoder_type="standard",
            decoder_type="standard", resample_filter=[1, 1], dropout=0.0, label_dropout=0, r_timestep=False, drop_precond=None)
DIT_S = dict(hidden_size=384, depth=12, num_heads=6)
WAN = dict(num_attention_heads=2, attention_head_dim=128, text_dim=128, ffn_dim=512, num_layers=2, chunk_size=2, total_num_frames=6)
NAN = float("nan")


def dev():
    return torch.device("cuda:0")


def rnd(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dev())


def dptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else None)


def darr(v):
    return (ctypes.c_double * len(v))(*[float(x) for x in v])


def cur_stream():
    return ctypes.c_void_p(torch.cuda.current_stream(dev()).cuda_stream)


class counted:
    """`with counted() as c:` - c.captures / c.launches of the calls inside."""

    def __enter__(self):
        self.c0, self.n0 = _lib.graph_stats()
        return self

    def __exit__(self, *exc):
        c, n = _lib.graph_stats()
        self.captures, self.launches = c - self.c0, n - self.n0


# ---- the entry points on buffers the test owns ----------------------------------------------------------------------------------
class Loop:
    """One handle's sampler entry point with its buffers.  `loop(graph, **changes)` runs it with `defaults` + `changes` and returns a
    copy of the result; `fill(k)` overwrites the contents of every input buffer; `graphs`: the graphs one call launches."""
    graphs = 1
    two_step = dict(tl=[0.999, 0.4, 0.0])

    def invalidate(self):
        """Leave graphs of another step count in the cache: the next call of any test is a miss whatever ran before."""
        self(True, **self.one_step)

    def __call__(self, graph, **kw):
        with torch.inference_mode():
            return self.run(graph, **{**self.defaults, **kw})


class UNetLoop(Loop):
    """fg_sampler_run / fg_edm2_sampler_run (one signature)."""
    one_step = dict(tl=[80.0, 0.0])
    two_step = dict(tl=[80.0, 2.0, 0.0])
    other_tl = dict(tl=[60.0, 7.0, 0.9, 0.0])

    def __init__(self, net, entry, res, B=2):
        self.net, self.entry, self.B = net, entry, B
        self.noise, self.labels = torch.empty(B, 3, res, res, device=dev()), torch.empty(B, 10, device=dev())
        self.eps, self.out, self.out2 = torch.empty(2, B, 3, res, res, device=dev()), torch.empty_like(self.noise), torch.empty_like(self.noise)
        self.defaults = dict(tl=[80.0, 9.0, 1.2, 0.0], stype="sde", seed=5, inject=True, batch=B, alt=False)
        self.fill(0)

    def fill(self, k):
        self.noise.copy_(rnd(self.noise.shape, 100 + k))
        self.labels.copy_(torch.nn.functional.one_hot((torch.arange(self.B) + 3 * k) % 10, 10).float())
        self.eps.copy_(rnd(self.eps.shape, 200 + k))

    def run(self, graph, tl, stype, seed, inject, batch, alt):
        dt, h = self.net._engine(dev())  # (binds and packs again when the weights changed; train() / eval())
        ws = self.net._workspace(dt, h, self.B, dev())
        out = self.out2 if alt else self.out
        out.fill_(NAN)
        _lib.check(getattr(_lib.lib(), self.entry)(
            h, dptr(self.noise), dptr(self.labels), darr(tl), len(tl) - 1, _lib.SAMPLE_TYPES[stype], _lib.FG_LOOP_X0,
            dptr(self.eps if inject else None), ctypes.c_uint64(seed), dptr(out), batch, dptr(ws), ws.numel(), int(graph), cur_stream()))
        return out[:batch].clone()


class DitLoop(Loop):
    """fg_dit_sampler_run: the x0, MeanFlow and Euler loops."""
    one_step = dict(tl=[0.999, 0.0])
    other_tl = dict(tl=[0.95, 0.6, 0.2, 0.0])

    def __init__(self, net, B=2):
        self.net, self.B = net, B
        self.noise = torch.empty(B, 4, 32, 32, device=dev())
        self.cls, self.neg = torch.empty(B, dtype=torch.int64, device=dev()), torch.empty(B, dtype=torch.int64, device=dev())
        self.eps, self.out, self.out2 = torch.empty(2, B, 4, 32, 32, device=dev()), torch.empty_like(self.noise), torch.empty_like(self.noise)
        self.defaults = dict(tl=[0.999, 0.7, 0.3, 0.0], stype="sde", loop="x0", seed=5, inject=True, batch=B, alt=False, guided=False, scale=2.5)
        self.fill(0)

    def fill(self, k):
        self.noise.copy_(rnd(self.noise.shape, 300 + k))
        self.cls.copy_((torch.arange(self.B) * 37 + 11 * k + 3) % 1000)
        self.neg.copy_(torch.full((self.B,), 1000) if k == 0 else (torch.arange(self.B) * 5 + k) % 1000)  # 1000: the unconditional row
        self.eps.copy_(rnd(self.eps.shape, 400 + k))

    def run(self, graph, tl, stype, loop, seed, inject, batch, alt, guided, scale):
        net, L = self.net, _lib.lib()
        dt, h = net._engine(dev())
        ws = net._workspace(dt, L.fg_dit_sampler_workspace_bytes(h, self.B, 1), dev())  # (room for the guided call: one address)
        sc = _lib.fg_dit_sampler_config()
        sc.t_scale, sc.guidance_scale = float(net.noise_scheduler.num_steps), float(scale if guided else 1.0)
        sc.use_sit_convention, sc.time_cond_diff, sc.net_pred_flow, sc.schedule = 0, 0, 1, _lib.FG_SCHEDULE_RF
        out = self.out2 if alt else self.out
        out.fill_(NAN)
        _lib.check(L.fg_dit_sampler_run(
            h, ctypes.byref(sc), dptr(self.noise), dptr(self.cls), dptr(self.neg if guided else None), darr(tl), len(tl) - 1,
            _lib.SAMPLE_TYPES[stype], _lib.LOOP_KINDS[loop], dptr(self.eps if inject else None), ctypes.c_uint64(seed), dptr(out), batch, dptr(ws),
            ws.numel(), int(graph), cur_stream()))
        return out[:batch].clone()


class WanLoop(Loop):
    """The buffers of the two video loops: latents (the loops run in place: every call starts from a copy of `src`), noise videos, two
    text conditions of 16 and 24 tokens for 2 B rows (the guided call's stacked [cond; neg])."""
    graphs = 2
    C, H, W, FMAX = 16, 16, 24, 6

    def __init__(self, net, B=2):
        self.net, self.B, self.h = net, B, net._h
        n = B * self.C * self.FMAX * self.H * self.W
        self.src, self.x, self.x2 = (torch.empty(n, device=dev()) for _ in range(3))
        self.eps = torch.empty(3 * n, device=dev())
        self.text = {16: torch.empty(2 * B, 16, 128, device=dev()), 24: torch.empty(2 * B, 24, 128, device=dev())}
        self.fill(0)

    def fill(self, k):
        self.src.copy_(rnd(self.src.shape, 500 + k) * 0.999)
        self.eps.copy_(rnd(self.eps.shape, 600 + k))
        for n, t in self.text.items():
            t.copy_(rnd(t.shape, 700 + n + k))

    def workspace(self):
        L, h, B = _lib.lib(), self.h, self.B
        self.net._bind(dev())  # (binds and packs again when the weights changed)
        need = max(max(L.fg_wan_sampler_workspace_bytes(h, B, f, self.H, self.W),
                       L.fg_wan_guided_sampler_workspace_bytes(h, B, f, self.H, self.W, 4, 1)) for f in (3, 4, 5))  # (one address for every call)
        return self.net._eng.workspace(self.net._cfg.compute_dtype, need, dev())

    def latents(self, batch, frames, alt):
        n = batch * self.C * frames * self.H * self.W
        x = (self.x2 if alt else self.x)[:n]
        (self.x2 if alt else self.x).fill_(NAN)
        x.copy_(self.src[:n])
        return x

    def set_text(self, rows, length, ws):
        _lib.check(_lib.lib().fg_wan_set_text(self.h, dptr(self.text[length]), rows, length, dptr(ws), ws.numel(), cur_stream()))

    def forward_probe(self):
        """Two plain network calls on the handle as the loops left it: chunk 0 with store_kv, chunk 1 over the stored rows."""
        L, B, ws = _lib.lib(), self.B, self.workspace()
        with torch.inference_mode():
            self.set_text(B, 16, ws)
            x = self.latents(B, 5, False).view(B, self.C, 5, self.H, self.W)
            outs = []
            for a, b, store in ((0, 3, 1), (3, 5, 0)):
                xc = x[:, :, a:b].contiguous()
                ts = torch.full((B, b - a), 500.0, device=dev())
                out = torch.full_like(xc, NAN)
                _lib.check(L.fg_wan_forward(self.h, dptr(xc), dptr(ts), dptr(out), B, b - a, self.H, self.W, a, store, dptr(ws), ws.numel(), cur_stream()))
                outs.append(out)
            _lib.check(L.fg_wan_clear_caches(self.h, cur_stream()))
        return outs


class WanStudentLoop(WanLoop):
    """fg_wan_sampler_run."""
    one_step = dict(tl=[0.999, 0.0])
    other_tl = dict(tl=[0.95, 0.6, 0.2, 0.0])

    def __init__(self, net, B=2):
        super().__init__(net, B)
        self.defaults = dict(tl=[0.999, 0.7, 0.3, 0.0], stype="ode", seed=5, inject=True, batch=B, alt=False, cn=0.0, exits=None, prefill=0,
                             frames=5, text=16)

    def run(self, graph, tl, stype, seed, inject, batch, alt, cn, exits, prefill, frames, text):
        L, net, ws = _lib.lib(), self.net, self.workspace()
        self.set_text(batch, text, ws)
        x = self.latents(batch, frames, alt)
        sc = _lib.fg_wan_sampler_config()
        sc.t_scale, sc.context_noise, sc.net_pred_flow = float(net.noise_scheduler.num_steps), float(cn), 1
        sc.schedule, sc.prefill_frames = _lib.FG_SCHEDULE_RF, prefill
        ex = (ctypes.c_int * len(exits))(*exits) if exits is not None else None
        _lib.check(L.fg_wan_sampler_run(
            self.h, ctypes.byref(sc), dptr(x), darr(tl), len(tl) - 1, _lib.SAMPLE_TYPES[stype], ex, dptr(self.eps if inject else None),
            ctypes.c_uint64(seed), batch, frames, self.H, self.W, dptr(ws), ws.numel(), int(graph), cur_stream()))
        return x.clone()


class WanGuidedLoop(WanLoop):
    """fg_wan_guided_sampler_run: `tl` here is (steps, shift) of the flow-shift sigmas; the table carries the guidance scale."""
    one_step = dict(tl=(1, 5.0))
    two_step = dict(tl=(2, 5.0))
    other_tl = dict(tl=(3, 3.0), scale=2.5)

    def __init__(self, net, B=2):
        super().__init__(net, B)
        self.defaults = dict(tl=(3, 5.0), seed=5, inject=True, batch=B, alt=False, cn=0.0, frames=5, text=16, guided=True, scale=5.0)

    def run(self, graph, tl, seed, inject, batch, alt, cn, frames, text, guided, scale):
        L, net, ws = _lib.lib(), self.net, self.workspace()
        steps, shift = tl
        self.set_text(2 * batch if guided else batch, text, ws)
        x = self.latents(batch, frames, alt)
        sig = solvers.flow_shift_sigmas(steps, float(shift))
        table = solvers.multistep_table(sig, "unipc", float(scale) if guided else 1.0)
        t_net = torch.floor(sig[:-1] * 1000.0) / 1000.0
        sc = _lib.fg_wan_guided_sampler_config()
        sc.t_scale, sc.context_noise, sc.guidance = float(net.noise_scheduler.num_steps), float(cn), int(guided)
        _lib.check(L.fg_wan_guided_sampler_run(
            self.h, ctypes.byref(sc), dptr(x), darr(t_net.tolist()), darr(table.reshape(-1).tolist()), steps,
            dptr(self.eps if inject and cn > 0 else None), ctypes.c_uint64(seed), batch, frames, self.H, self.W, dptr(ws), ws.numel(), int(graph),
            cur_stream()))
        return x.clone()


# ---- one module and one Loop per family, built on first use ---------------------------------------------------------------------
def _song(**kw):
    net = EDMPrecond(**{**SONG, **kw})
    net.load_state_dict(edm_ref.random_state_dict(edm_ref.CIFAR10, seed=1234), strict=True)
    return net.to(dev()).eval().requires_grad_(False)


def _adm():
    net = EDMPrecond(**ADM.NARROW.kwargs())
    net.load_state_dict(ADM.random_state_dict(ADM.NARROW, seed=1234), strict=True)
    return net.to(dev()).eval().requires_grad_(False)


def _edm2():
    net = EDM2Precond(**E2.NARROW.kwargs())
    net.load_state_dict(E2.random_state_dict(E2.NARROW, seed=1234), strict=True)
    return net.to(dev()).eval().requires_grad_(False)


def _dit(**kw):
    cfg = dit_ref.DiTConfig(**DIT_S, **kw)
    net = DiT(**DIT_S, **kw)
    net.load_state_dict(dit_ref.random_state_dict(cfg, seed=77), strict=True)
    return net.to(dev()).eval().requires_grad_(False)


def _dit_small_r():
    kw = dict(hidden_size=384, depth=2, num_heads=6, r_timestep=True)
    net = DiT(**kw)
    net.load_state_dict(dit_ref.random_state_dict(dit_ref.DiTConfig(**kw), seed=78), strict=True)
    return net.to(dev()).eval().requires_grad_(False)


def _wan(seed=23):
    net = CausalWan(**WAN)
    net.load_state_dict(wan_ref.random_state_dict(wan_ref.TINY, seed), strict=True)
    return net.to(dev()).eval().requires_grad_(False)


MAKE = {
    "song": lambda: UNetLoop(_song(), "fg_sampler_run", 32),
    "adm": lambda: UNetLoop(_adm(), "fg_sampler_run", 64),
    "edm2": lambda: UNetLoop(_edm2(), "fg_edm2_sampler_run", 64),
    "dit": lambda: DitLoop(_dit()),
    "dit_r": lambda: DitLoop(_dit_small_r()),
    "wan": lambda: WanStudentLoop(_wan()),
    "wan_guided": lambda: WanGuidedLoop(_wan()),
}
FAMILIES = ["song", "adm", "edm2", "dit", "wan", "wan_guided"]
_LOOPS = {}


def loop_of(family):
    if family not in _LOOPS:
        _LOOPS[family] = MAKE[family]()
    return _LOOPS[family]


def equal(a, b):
    return a.shape == b.shape and bool(torch.isfinite(a).all()) and torch.equal(a, b)


# ---- a. capture, then hit --------------------------------------------------------------------------------------------------------
X0 = [dict(stype="sde"), dict(stype="ode"), dict(stype="sde", inject=False)]
KINDS = [(f, v) for f in ("song", "adm", "edm2", "dit") for v in X0]
KINDS += [("dit_r", dict(loop="meanflow", stype="sde")), ("dit_r", dict(loop="meanflow", stype="ode")),
          ("dit", dict(loop="euler", stype="ode", guided=True)), ("dit", dict(loop="euler", stype="ode"))]
KINDS += [("wan", dict(stype="ode")), ("wan", dict(stype="sde", cn=0.1)), ("wan", dict(stype="sde", inject=False)),
          ("wan", dict(stype="ode", exits=[0, 2]))]
KINDS += [("wan_guided", dict()), ("wan_guided", dict(guided=False)), ("wan_guided", dict(cn=0.1)), ("wan_guided", dict(cn=0.1, inject=False))]


@pytest.mark.parametrize("family,kind", KINDS, ids=lambda v: v if isinstance(v, str) else "-".join(f"{k}={x}" for k, x in v.items()) or "default")
def test_first_call_captures_and_the_second_replays(family, kind):
    loop = loop_of(family)
    loop.invalidate()
    eager = loop(False, **kind)
    with counted() as first:
        g1 = loop(True, **kind)
    with counted() as second:
        g2 = loop(True, **kind)
    assert (first.captures, first.launches) == (loop.graphs, loop.graphs)
    assert (second.captures, second.launches) == (0, loop.graphs)
    assert equal(g1, eager) and equal(g2, eager)


# ---- b. nothing is baked in by value -----------------------------------------------------------------------------------------------
INJECTED = {"song": dict(stype="sde"), "adm": dict(stype="sde"), "edm2": dict(stype="sde"), "dit": dict(stype="sde"),
            "wan": dict(stype="sde", cn=0.1), "wan_guided": dict(cn=0.1)}
DRAWN = {f: {**v, "inject": False} for f, v in INJECTED.items()}


@pytest.mark.parametrize("family", FAMILIES)
def test_replays_read_the_buffers_and_the_scalars_of_their_own_call(family):
    loop, kind = loop_of(family), INJECTED[family]
    loop.fill(0)
    loop.invalidate()
    seen = [loop(True, **kind)]  # the capture

    def replay(**kw):
        with counted() as c:
            got = loop(True, **{**kind, **kw})
        assert (c.captures, c.launches) == (0, loop.graphs), kw
        assert equal(got, loop(False, **{**kind, **kw})), kw
        assert all(not torch.equal(got, s) for s in seen), kw  # (the new values were read: no earlier result comes back)
        seen.append(got)

    loop.fill(1)  # other noise / latents, class ids or text, injected eps - in the buffers the graph was captured on
    replay()
    replay(**loop.other_tl)  # another t_list (the guided loop: another timestep list and solver table) of the same zero pattern
    loop.fill(0)
    # device-drawn noise: the seed is device memory too
    kind = DRAWN[family]
    seen = [loop(True, seed=11, **kind)]  # (a capture: the eps pointer of the key is null now)
    replay(seed=12)
    replay(seed=13, **loop.other_tl)


def test_dit_guided_euler_replays_read_the_negative_class_ids():
    loop, kind = loop_of("dit"), dict(loop="euler", stype="ode", guided=True)
    loop.fill(0)
    loop.invalidate()
    first = loop(True, **kind)
    loop.fill(1)
    with counted() as c:
        got = loop(True, scale=1.5, **kind)  # (the guidance scale is in the key: a capture)
    assert c.captures == 1 and equal(got, loop(False, scale=1.5, **kind))
    loop.neg.copy_(torch.tensor([7, 1000], device=dev()))
    with counted() as c:
        again = loop(True, scale=1.5, **kind)
    assert c.captures == 0 and equal(again, loop(False, scale=1.5, **kind)) and not torch.equal(again, got) and not torch.equal(got, first)
    loop.fill(0)


# ---- c. what must not be replayed ----------------------------------------------------------------------------------------------------
ZEROS = dict(tl=[0.999, 0.6, 0.0, 0.0])  # an interior zero (RF): step 1 does not re-noise
MISSES = {f: [("steps", {}, "two_step"), ("ode", {}, dict(stype="ode")), ("batch", {}, dict(batch=1)), ("out", {}, dict(alt=True))]
          for f in ("song", "adm", "edm2", "dit")}
MISSES["dit"] += [("zero pattern", {}, ZEROS), ("loop", dict(stype="ode"), dict(stype="ode", loop="euler")),
                  ("guided", dict(stype="ode", loop="euler"), dict(stype="ode", loop="euler", guided=True))]
MISSES["wan"] = [("steps", {}, "two_step"), ("sde", {}, dict(stype="sde")), ("batch", {}, dict(batch=1)), ("x", {}, dict(alt=True)),
                 ("zero pattern", dict(stype="sde"), dict(stype="sde", **ZEROS)), ("context_noise", dict(stype="sde"), dict(stype="sde", cn=0.1)),
                 ("context_noise value", dict(stype="sde", cn=0.1), dict(stype="sde", cn=0.2)), ("text length", {}, dict(text=24)),
                 ("prefill_frames", dict(frames=4), dict(frames=4, prefill=2)), ("frames", {}, dict(frames=4))]
MISSES["wan_guided"] = [("steps", {}, "two_step"), ("batch", {}, dict(batch=1)), ("x", {}, dict(alt=True)), ("context_noise", {}, dict(cn=0.1)),
                        ("text length", {}, dict(text=24)), ("guidance", {}, dict(guided=False)), ("frames", {}, dict(frames=4))]


@pytest.mark.parametrize("family,what", [(f, m[0]) for f in FAMILIES for m in MISSES[f]])
def test_a_changed_argument_is_captured_again(family, what):
    loop = loop_of(family)
    _, before, after = next(m for m in MISSES[family] if m[0] == what)
    after = getattr(loop, after) if isinstance(after, str) else after
    loop.invalidate()
    loop(True, **before)
    with counted() as c:
        got = loop(True, **after)
    assert c.captures >= 1 and c.launches == loop.graphs
    assert equal(got, loop(False, **after))
    with counted() as c:  # ... and the first arguments again: the single entry was replaced, so they are captured again too
        back = loop(True, **before)
    assert c.captures >= 1 and equal(back, loop(False, **before))


def test_wan_exit_step_of_one_chunk_recaptures_that_chunk_only():
    loop = loop_of("wan")
    loop.invalidate()
    loop(True, exits=[2, 2])
    for exits, chunk_graphs in (([2, 1], 1), ([0, 1], 1), ([0, 1], 0), ([1, 2], 2)):
        with counted() as c:
            got = loop(True, exits=exits)
        assert (c.captures, c.launches) == (chunk_graphs, 2), exits
        assert equal(got, loop(False, exits=exits)), exits


@pytest.mark.parametrize("family", ["song", "edm2"])
def test_train_eval_flip_with_sigma_shift_is_captured_again(family):
    """sigma_shift applies in eval mode only and is baked into the launches: with every buffer the same a train() / eval() flip must not
    replay the graph of the other mode."""
    if family == "song":
        loop = UNetLoop(_song(sigma_shift=0.05), "fg_sampler_run", 32)
    else:
        net = EDM2Precond(**E2.NARROW.kwargs(), sigma_shift=0.05)
        net.load_state_dict(E2.random_state_dict(E2.NARROW, seed=1234), strict=True)
        loop = UNetLoop(net.to(dev()).eval().requires_grad_(False), "fg_edm2_sampler_run", 64)
    runs = []
    for training in (False, True, False):
        loop.net.train(training)
        with counted() as c:
            runs.append(loop(True))
        assert c.captures == 1, training
        assert equal(runs[-1], loop(False)), training
    assert not torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])


# ---- d. one chunk replays, the other is captured ---------------------------------------------------------------------------------------
def test_wan_mixed_hit_and_miss_in_one_call_and_the_handle_afterwards():
    """Chunk 0 replays - its cache bookkeeping (`stored_rows`) is applied by hand - and chunk 1 is captured on top of it; then the other
    way round.  Afterwards the handle answers plain network calls with the bits of a handle that only ever ran eager."""
    loop, eager_only = loop_of("wan"), WanStudentLoop(_wan())
    loop.fill(0)
    loop.invalidate()
    loop(True, exits=[2, 2])
    with counted() as c:
        got = loop(True, exits=[2, 0])
    assert (c.captures, c.launches) == (1, 2) and equal(got, eager_only(False, exits=[2, 0]))
    with counted() as c:
        got = loop(True, exits=[1, 0])  # chunk 0 captured, chunk 1 replayed
    assert (c.captures, c.launches) == (1, 2) and equal(got, eager_only(False, exits=[1, 0]))
    with counted() as c:
        got = loop(True, exits=[1, 0], stype="sde", cn=0.1)
    assert c.captures == 2 and equal(got, eager_only(False, exits=[1, 0], stype="sde", cn=0.1))
    for a, b in zip(loop.forward_probe(), eager_only.forward_probe()):
        assert equal(a, b)


def test_wan_guided_mixed_hit_and_miss_in_one_call_and_the_handle_afterwards():
    """The guided loop's key has nothing of its own per chunk but the frames: a three-frame call in between replaces chunk 0's graph,
    so that the next five-frame call captures chunk 0 and replays chunk 1 after it."""
    loop, eager_only = loop_of("wan_guided"), WanGuidedLoop(_wan())
    loop.fill(0)
    loop.invalidate()
    five = loop(True)
    with counted() as c:
        three = loop(True, frames=3)
    assert (c.captures, c.launches) == (1, 1) and equal(three, eager_only(False, frames=3))
    with counted() as c:
        got = loop(True)
    assert (c.captures, c.launches) == (1, 2) and equal(got, five) and equal(got, eager_only(False))
    with counted() as c:
        got = loop(True, **loop.other_tl)
    assert (c.captures, c.launches) == (0, 2) and equal(got, eager_only(False, **loop.other_tl))
    for a, b in zip(loop.forward_probe(), eager_only.forward_probe()):
        assert equal(a, b)


# ---- e. interleaving -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_eager_and_graph_calls_and_two_shapes_interleaved(family):
    loop, kind = loop_of(family), INJECTED[family]
    loop.invalidate()
    runs = [loop(graph, **kind) for graph in (False, True, False, True)]
    assert all(equal(r, runs[0]) for r in runs)
    small = loop(False, batch=1, **kind)
    for batch, want in ((1, small), (2, runs[0]), (1, small)):  # shapes A, B, A on the single-entry cache
        with counted() as c:
            got = loop(True, batch=batch, **kind)
        assert (c.captures, c.launches) == (loop.graphs, loop.graphs) and equal(got, want), batch


def test_wan_cache_tag_switched_between_two_student_calls():
    loop, L = loop_of("wan"), _lib.lib()
    loop.invalidate()
    want = loop(False)
    assert equal(loop(True), want)
    _lib.check(L.fg_wan_select_cache_tag(loop.h, 1))
    _lib.check(L.fg_wan_select_cache_tag(loop.h, 0))
    with counted() as c:
        got = loop(True)
    assert c.captures == 0 and equal(got, want)
    # ... and the loop on tag 1's own caches, then on tag 0's again
    _lib.check(L.fg_wan_select_cache_tag(loop.h, 1))
    try:
        with counted() as c:
            got = loop(True)
        assert c.captures == 2 and equal(got, want) and equal(loop(False), want)
    finally:
        _lib.check(L.fg_wan_select_cache_tag(loop.h, 0))
    assert equal(loop(True), want)


# ---- f. weights changed between two graph calls ------------------------------------------------------------------------------------------
def _touched(family, net):
    names = [n for n, _ in net.named_parameters()]
    if family in ("song", "adm", "edm2"):  # one 3 x 3 conv
        return next(n for n, p in net.named_parameters() if p.ndim == 4 and p.shape[-1] == 3 and p.shape[1] > 3)
    return next(n for n in names if "blocks.0." in n and n.endswith("weight") and dict(net.named_parameters())[n].ndim == 2)


@pytest.mark.parametrize("family", FAMILIES)
def test_weights_updated_in_place_between_two_graph_calls(family):
    """(What a pack does to the buffers a cached graph names was read first: the U-Nets' packs drop the graph; the DiT's and the video
    DiT's packs allocate on the first pack only and write in place afterwards.)"""
    loop, kind = loop_of(family), INJECTED[family]
    loop.invalidate()
    before = loop(True, **kind)
    p = dict(loop.net.named_parameters())[_touched(family, loop.net)]
    p = p[:, : p.shape[1] // 2]  # (half of every row: EDM2 normalises each output channel's weights, a common factor would cancel)
    with torch.no_grad():
        p.mul_(0.5)
    try:
        after = loop(True, **kind)
        assert equal(after, loop(False, **kind)) and not torch.equal(after, before)
    finally:
        with torch.no_grad():
            p.mul_(2.0)
    assert equal(loop(True, **kind), before)


# ---- the public API has to replay -----------------------------------------------------------------------------------------------------
def _twice(call):
    """`call()` three times - eager, graph, graph - on freshly allocated inputs, with the earlier calls' tensors still alive (the
    allocator cannot hand the same addresses out again): the third is a replay, and every result is the eager one."""
    alive = []
    with torch.inference_mode():
        eager, keep = call(False)
    alive.append(keep)
    with torch.no_grad(), counted() as first:  # (no_grad after inference_mode: the handle's own tensors must take both)
        a, keep = call(True)
    alive.append(keep)
    with torch.inference_mode(), counted() as second:
        b, keep = call(True)
    assert first.launches == second.launches >= 1
    assert second.captures == 0, f"the second call captured {second.captures} graph(s)"
    assert equal(a, eager) and equal(b, eager)
    return a, b


@pytest.mark.parametrize("family", ["song", "adm", "edm2"])
def test_unet_few_step_sample_replays_on_fresh_tensors(family):
    net, res = loop_of(family).net, 32 if family == "song" else 64
    noise, eps = rnd((2, 3, res, res), 1), rnd((2, 2, 3, res, res), 2)
    tl = [80.0, 9.0, 1.2, 0.0]

    def call(graph):
        args = noise.clone(), torch.nn.functional.one_hot(torch.tensor([1, 7]), 10).float().to(dev()), eps.clone()
        return net.few_step_sample(args[0], args[1], tl, sample_type="sde", eps=args[2], use_graph=graph), args

    a, b = _twice(call)
    assert a.data_ptr() != b.data_ptr()  # each result is the caller's own tensor
    out, cond = torch.empty_like(noise), torch.nn.functional.one_hot(torch.tensor([1, 7]), 10).float().to(dev())
    assert net.few_step_sample(noise, cond, tl, sample_type="sde", eps=eps, out=out) is out and equal(out, a)  # `out=` as before


@pytest.mark.parametrize("method", ["few_step_sample", "sample", "generator_fn"])
def test_dit_methods_replay_on_fresh_tensors(method):
    net = loop_of("dit").net
    noise, eps = rnd((2, 4, 32, 32), 1), rnd((2, 2, 4, 32, 32), 2)

    def call(graph):
        cond = torch.nn.functional.one_hot(torch.tensor([3, 500]), 1000).float().to(dev())
        neg = torch.zeros(2, 1000, device=dev())
        args = noise.clone(), cond, neg, eps.clone()
        if method == "few_step_sample":
            out = net.few_step_sample(args[0], cond, [0.999, 0.7, 0.3, 0.0], sample_type="sde", eps=args[3], use_graph=graph)
        elif method == "sample":
            out = net.sample(args[0], condition=cond, neg_condition=neg, guidance_scale=2.5, num_steps=3, use_graph=graph)
        else:
            out = FastGenModel.generator_fn(net, args[0], student_sample_steps=3, condition=cond, student_sample_type="sde", eps=args[3],
                                            use_graph=graph)
        return out, args

    a, b = _twice(call)
    assert a.data_ptr() != b.data_ptr()


@pytest.mark.parametrize("method", ["student_sample", "sample"])
def test_wan_methods_replay_on_fresh_tensors(method):
    net = loop_of("wan").net
    net.clear_caches()
    B, F, H, W = 2, 5, 16, 24
    lat, text, neg = rnd((B, 16, F, H, W), 1) * 0.999, rnd((B, 16, 128), 2), rnd((B, 16, 128), 3)
    eps = rnd((3, B, 16, F, H, W), 4)

    def call(graph):
        x, args = lat.clone(), (text.clone(), neg.clone(), eps.clone())
        if method == "student_sample":
            out = net.student_sample(x, [0.999, 0.7, 0.3, 0.0], args[0], sample_type="sde", context_noise=0.1, eps=args[2], use_graph=graph)
        else:
            out = net.sample(x, args[0], args[1], sample_steps=3, context_noise=0.1, eps=args[2][0], use_graph=graph)
        assert out is x  # the caller's latents, overwritten
        return out, (x,) + args

    _twice(call)
