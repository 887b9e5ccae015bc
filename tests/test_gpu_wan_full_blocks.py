"""Per-block and per-op parity of the BIDIRECTIONAL video DiT call (`fg_wan_forward_full`: engine_wan.inc's third mode of wan_forward -
one attention launch over all frames, `r_frames`, `skip_layers`, the frame count bounded by the RoPE table) against the oracle's pieces
(oracle/wan_ref.py) in fp64, with the machinery of tests/test_gpu_wan_blocks.py (imported, not copied: `run_case` with calls of kind
"full"), per (sample, frame), per (sample, head), per last ragged query tile and per (sample, query, head).

`fg_wan_forward_full_features` taps what fg_wan_forward_features taps, and `tproj`: timestep_proj with the r term added.  Conventions as
in the causal file: the engine through the C ABI, 2-layer networks (3 where a block is skipped), text_dim 64, 37 text tokens, every
sample its own x and text, Q_GAIN on norm_q, increments compared instead of streams, block i run by the oracle on the GPU's own block
input; at B >= 9 samples {0, 1, 7, 8, B - 1}, always all frames.  EVERY FRAME HAS ITS OWN t AND ITS OWN r (`_inputs`: no two of the
2 B F values coincide, t - r > 0) - the module `Wan.forward` only ever hands the engine one t and one r per sample, so an engine that
indexed either by sample passes every network-level test.  rope_max_seq_len is the frame count: the last frame sits on the table's last
row (the 5-, 10- and 11-frame cases of 16 x 24 latents need the 12 rows their 12 grid columns index: the engine refuses a smaller table).  total_num_frames = 3 and chunk_size = 2 wherever the handle takes them: every call runs past the causal calls' cache plan.

The matrix is chosen by the launch plan of its self-attention (Lq == Lkv), which tests/test_wan_full_ref.py::test_full_cases_reach_the_planned_kernels holds to
`fg_op_attention_plan` without a GPU - every form named in PLANS is run: fa_kernel with one split, with the cost model's key split (with
and without a batch), sample-major; fa2_kernel with the uneven cut at B = 2 and at B = 9 just past the sample-major limit (where the
cross-attention leaves that map too), even with one split and with three (merge pass).  The oracle of the cases of >= 960 tokens runs
in fp64 on the device.

Checks per call: temb (with r: temb + remb) and tproj against the fp64 embedders on the fp32 timesteps the kernels read (fp32(t - r)
for "diff"); tokens_out element-wise on its derived bound; per block attn1, attn1/row, inc1, attn2, attn2/row, inc2, ffn; out on the
GPU's last stream; the tapped `out` torch.equal to fg_wan_forward_full's; a second tapped call with the same x_ffn.  A block behind a
skipped one is checked against the oracle run on the tap of the block before the skipped one.  FP8: only the `out` equality.

Bounds: TOL, TOK_ULP, TOK_ABS and MUTANT_FACTOR of the causal file; tproj takes temb's (both are fp32 linears of the same depth).
The comment above `report` records what an MI355X gave over this matrix: every quantity stays inside the causal bounds.

Mutants, each built in fp64 from the oracle alone and missing its bound MUTANT_FACTOR times over: (a), (b), (d), (e), (f) of the causal
file, and
  (m) the block-causal mask of the config's chunk_size in place of full attention (attn1, worst (sample, frame | head));
  (n) the temporal RoPE index clamped at total_num_frames - 1 (attn1);
  (o) r rolled by one frame within each sample - what an r indexed per sample instead of per (sample, frame) amounts to - on temb and
      on tproj, in every row;
  (p) the wrong r term - r ignored, time_cond_type swapped, "proj only" (r_timestep_proj added, remb not) - on temb / tproj in every
      row, whichever it changes, and again through what reads it: inc1 and ffn (the gates and the MLP's scale / shift of the wrong
      tproj), the output layer ("proj only" changes temb alone, which only the output modulation reads);
  (q) skip ignored: the reference runs the skipped blocks, on inc1 of the next block that ran (every granule), or on `out` when the
      skipped block is the last.
tests/test_wan_full_ref.py::test_full_block_mutants_stand_apart shows without a GPU that (m) - (q) stand 5 x their bounds from the
unmutated oracle at these seeds."""
import pytest

from test_gpu_wan_blocks import MUTANT_FACTOR, TOK_ABS, TOK_ULP, TOL, Case, Gpu, run_case  # noqa: F401

from fastgen_amd._lib import FG_FA_TILE128, FG_FA_WIDE, FG_FA_WIDE_CUT

pytestmark = pytest.mark.gpu

TOL_FULL = dict(TOL, tproj=TOL["temb"])


def _full(frames, r=False, skip=()):
    return ("full", 0, frames, 0, r, tuple(skip))


def _case(frames, **kw):
    kw.setdefault("calls", (_full(frames),))
    kw.setdefault("total", 3)
    kw.setdefault("chunk", 2)
    lat = kw.get("lat", Case.lat)
    return Case(rope_max=max(frames, lat[0] // 2, lat[1] // 2), **kw)  # (the table must also hold the grid's rows and columns: 12 at 16 x 24)


BIG = dict(lat=(16, 24), device_oracle=True)  # 96 tokens per frame
CASES = {
    # 7 frames on a cache plan of 3, chunks of 2: a leftover chunked mask or a clamped RoPE / cache plan would show
    "F105": _case(7),
    "F555": _case(37),                       # the cost model's key split with Lq == Lkv, ragged tiles
    "F720-B3": _case(48, B=3),               # the same with a batch
    "F960-B9": _case(10, B=9, **BIG),        # sample-major self-attention, straddling the group of 8
    "F1152-B2": _case(12, B=2, **BIG),       # fa2_kernel's cut at batch 2, 4.5 query tiles of 256
    "F1056-B9": _case(11, B=9, **BIG),       # B >= 8 just past the sample-major limit; the cross-attention leaves that map
    "F1152-B26": _case(12, B=26, **BIG),     # fa2_kernel even, one split (P > 248)
    "F2400-B13": _case(25, B=13, **BIG),     # fa2_kernel even, three splits chosen by the cost model, merge pass
    "F105-D384": _case(7, heads=3, ffn=1024),
    "F105-D1536": _case(7, heads=12, ffn=8960),
    "F105-C8": _case(7, B=2, chans=8),       # generic patch-embed kernel, C != 16 in the final kernel
    # the r_embedder (a `Wan` handle: chunk_size = total_num_frames = 1), r_frames given, then the same handle with r_frames null
    "R-diff": _case(5, B=2, lat=(16, 24), r="diff", total=1, chunk=1, calls=(_full(5, r=True), _full(5))),
    "R-abs": _case(5, B=2, lat=(16, 24), r="abs", total=1, chunk=1, calls=(_full(5, r=True), _full(5))),
    "SKIP": _case(5, B=2, lat=(16, 24), layers=3, calls=(_full(5, skip=(1,)), _full(5, skip=(0, 2)))),
    "FP8": _case(5, B=2, lat=(16, 24), dtype="fp8"),
}

# name: (self-attention plan, cross-attention plan) as (kernel form, splits, cut, sample-major); Lq == Lkv == frames x frame tokens, ldk = D
# for the first, Lkv = 37 and ldk = 2 D (k | v rows) for the second, both with scratch
_T1 = (FG_FA_TILE128, 1, 0, 0)
PLANS = {
    "F105": (_T1, _T1), "F555": ((FG_FA_TILE128, 2, 0, 0), _T1), "F720-B3": ((FG_FA_TILE128, 2, 0, 0), _T1),
    "F960-B9": ((FG_FA_TILE128, 1, 0, 1), (FG_FA_TILE128, 1, 0, 1)), "F1152-B2": ((FG_FA_WIDE_CUT, 2, 18, 0), _T1),
    "F1056-B9": ((FG_FA_WIDE_CUT, 2, 17, 0), _T1), "F1152-B26": ((FG_FA_WIDE, 1, 0, 0), _T1), "F2400-B13": ((FG_FA_WIDE, 3, 0, 0), _T1),
    "F105-D384": (_T1, _T1), "F105-D1536": (_T1, _T1), "F105-C8": (_T1, _T1), "R-diff": (_T1, _T1), "R-abs": (_T1, _T1), "SKIP": (_T1, _T1),
    "FP8": (_T1, _T1),
}

# Worst values measured on an MI355X over this matrix, (relative L2, max |err| / max |ref|) with the case that set each, beside the causal
# file's bounds (TOL = twice the causal matrix's worst) - none of them is exceeded, so no bound is widened here:
#   temb 1.44e-5 / 1.87e-5 (F720-B3; bound 2.2e-5 / 2.7e-5); tproj 1.42e-5 / 1.94e-5 (F720-B3; temb's bound);
#   attn1 per (sample, frame | head | last tile) 1.06e-2 / 2.39e-2 (F555; 2.4e-2 / 5.8e-2), per (sample, query, head) 3.09e-2 (F105-D384)
#   / 4.12e-2 (F1152-B2; 8.8e-2 / 9.5e-2); inc1 2.37e-2 (F2400-B13) / 2.53e-2 (F720-B3; 4.4e-2 / 4.5e-2); attn2 4.90e-3 (F105-D384) /
#   1.11e-2 (F1152-B2; 1.05e-2 / 2.3e-2), per query 1.04e-2 (F2400-B13) / 1.39e-2 (R-abs; 2.1e-2 / 2.7e-2); inc2 8.38e-3 (R-diff) /
#   1.75e-2 (F1056-B9; 1.75e-2 / 3.7e-2); ffn 1.66e-2 (F2400-B13) / 1.96e-2 (F720-B3; 3.5e-2 / 4.5e-2); out 1.38e-7 (F105-D1536) /
#   2.69e-7 (F720-B3; 4e-7 / 5.5e-7); tokens_out 0.985 of its derived bound (F2400-B13).  Attention over 2400 keys (three merged
#   splits) sits where 105 keys sit: the per-query error is the bf16 rounding of P and V, not a function of the key count.
# Smallest mutant distance, as a multiple of the bound of the quantity it is checked on: (a) 22, (b) 25, (d) 59, (e) 13 (F2400-B13: 17
# of 2400 keys), (f) 26, (m) 23 (SKIP), (n) 11.5 (F105), (o) 3.1e4, (p) on temb / tproj 2.7e4 ... 4e4, through inc1 / ffn 18 ... 38,
# "proj only" on out 1.1e6, (q) 21 on inc1 and 6.8e5 on out.


def report(name, rep):
    print(f"\n[wan-full-blocks] {name} " + " ".join(f"{k}={v[0]:.2e}/{v[1]:.2e}" for k, v in rep.worst.items()))
    print(f"[wan-full-blocks] {name} mutants (x bound) " + " ".join(f"{k}={v:.3g}" for k, v in rep.mut.items()))


@pytest.mark.parametrize("name", list(CASES))
def test_full_blocks(name):
    rep = run_case(CASES[name], Gpu, TOL_FULL)
    report(name, rep)
    assert not rep.bad, rep.bad
