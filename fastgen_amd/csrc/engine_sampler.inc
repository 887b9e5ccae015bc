// Sampler loops of the transformer networks as library calls, each replayed as hipGraphs (SURVEY 8(a) rows `generator_fn` /
// `_student_sample_loop` for the DiT and causal-video-DiT networks; north_star: "the outer 1-4-step sampler loop is hipGraph-captured"):
//   fg_dit_sampler_run   FastGenModel._student_sample_loop (methods/model.py:315-372), MeanFlowModel._student_sample_loop
//                        (consistency_model/mean_flow.py:336-381) and DiT._sample_flow (DiT/network.py:605-651) around fg_dit_forward
//   fg_wan_sampler_run   CausVidModel._student_sample_loop (distribution_matching/causvid.py:87-185), the segment loop of
//                        generator_fn_extrapolation (:188-397) and SelfForcingModel.rollout_with_gradient's no-grad form
//                        (self_forcing.py:92-241) around fg_wan_forward: per chunk N x {x0 prediction; re-noise}, then the cache-fill call
//   fg_wan_full_sampler_run / fg_wan_full_guided_sampler_run   the bidirectional video DiT's student loops and guided teacher loop
//                        over the whole video (at the end of this file)
// Textually included by engine.hip behind engine_dit.inc / engine_wan.inc; the argument check, scalar ring, graph cache and the
// student loops (x0_loop, meanflow_loop, renoise_x0) are engine.hip's.  The reference's host syncs (`t_next > 0` on a device tensor,
// `assert is_t_valid(t)` in every schedule call, `rescale_t`) are hoisted to host scalars checked once per call; timesteps and the RNG
// seed live in device memory, so a captured graph is replayed with new values.
}  // extern "C" (reopened below)

namespace {

// ---- DiT ----------------------------------------------------------------------------------------------------------------------
struct DitLoopWs {
    bool guided = false;  // the plan's input: room for the doubled batch of a guided FG_LOOP_EULER call
    DitWs net;
    float *x, *v, *pred, *eps, *te, *re;
    double* tl;
    uint64_t* seed;
    int64_t* cls2;
};

size_t dit_sampler_plan(const fg_dit* h, int B, Arena& A, DitLoopWs& w) {
    const int Be = w.guided ? 2 * B : B;
    dit_plan(h, Be, A, w.net);
    const size_t per = (size_t)h->cfg.in_channels * h->cfg.input_size * h->cfg.input_size;
    w.x = A.get<float>(per * Be);
    w.v = A.get<float>(per * Be);
    w.pred = A.get<float>(per * B);
    w.eps = A.get<float>(per * B);
    w.te = A.get<float>(Be);
    w.re = A.get<float>(Be);
    w.tl = A.get<double>(ScalarRing::kDoubles);
    w.seed = A.get<uint64_t>(2);
    w.cls2 = A.get<int64_t>(2 * (size_t)B);
    return (A.off + 255) & ~(size_t)255;
}

int dit_enqueue_sampler(fg_dit* h, const fg_dit_sampler_config& sc, const float* noise, const int64_t* cls, const int64_t* neg, const double* t_list,
                        int steps, int type, int loop, const float* eps, float* out, int B, DitLoopWs& w, hipStream_t s) {
    const fg_dit_config& c = h->cfg;
    const int64_t total = (int64_t)B * c.in_channels * c.input_size * c.input_size;
    const int Be = w.guided ? 2 * B : B;
    const float sign = (sc.use_sit_convention && sc.net_pred_flow) ? -1.0f : 1.0f;  // DiT/network.py:555-558
    const int64_t* ids = w.guided ? w.cls2 : cls;
    // the network on w.x at t_i into v; ri: MeanFlow's r (-1: 0, else t_list[ri]), -2: none
    auto net = [&](int i, int ri, float* v) -> int {
        HIP_TRY(launch_embed_times(w.tl, i, 0.0, ri, 0.0, sc.t_scale, sc.use_sit_convention, sc.time_cond_diff, 0, w.te, w.re, Be, s));
        return dit_forward(h, w.x, w.te, ri == -2 ? nullptr : w.re, ids, v, nullptr, Be, w.net, s);
    };
    const StudentLoop L{noise, t_list, steps, type, sc.schedule, total, w.x, w.eps, eps, w.tl, w.seed, out, s};
    if (loop == FG_LOOP_X0)  // the network's flow prediction -> x0 (convert_model_output, :560-566)
        return x0_loop(L, w.pred, [&](int i, float* pred) -> int {
            const int rc = net(i, -2, w.v);
            if (rc) return rc;
            if (sc.net_pred_flow) HIP_TRY(launch_flow_to_x0(w.x, w.v, w.tl, i, sign, pred, total, s));
            else HIP_TRY(hipMemcpyAsync(pred, w.v, sizeof(float) * total, hipMemcpyDeviceToDevice, s));
            return FG_OK;
        });
    if (loop == FG_LOOP_MEANFLOW)  // r: 0 for the 'sde' jump to the data end, the next timestep for 'ode' (mean_flow.py:362-368)
        return meanflow_loop(L, w.v, [&](int i, float* u) { return net(i, type == FG_SAMPLE_SDE ? -1 : i + 1, u); });
    // FG_LOOP_EULER
    HIP_TRY(launch_latents(noise, 0.0, w.tl, 0, w.x, total, s));  // latents = noise * sigma(t_0), noise_schedule.py:72-88
    if (w.guided) {  // the doubled batch of the guided call: [x | x], [neg_condition | condition] (:636-640)
        HIP_TRY(hipMemcpyAsync(w.x + total, w.x, sizeof(float) * total, hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipMemcpyAsync(w.cls2, neg, sizeof(int64_t) * B, hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipMemcpyAsync(w.cls2 + B, cls, sizeof(int64_t) * B, hipMemcpyDeviceToDevice, s));
    }
    for (int i = 0; i < steps; ++i) {
        const int rc = net(i, -2, w.v);
        if (rc) return rc;
        HIP_TRY(launch_euler_step(w.x, w.v, w.tl, i, (float)sc.guidance_scale, w.guided, sign, i == steps - 1 ? out : w.x,
                                  w.guided && i + 1 < steps ? w.x + total : nullptr, total, s));
    }
    return FG_OK;
}

}  // namespace

extern "C" {

size_t fg_dit_sampler_workspace_bytes(const fg_dit* h, int batch, int guided) {
    if (!h || batch <= 0) return 0;
    Arena A;
    A.dry = true;
    DitLoopWs w;
    w.guided = guided != 0;
    return dit_sampler_plan(h, batch, A, w);
}

int fg_dit_sampler_run(fg_dit* h, const fg_dit_sampler_config* sc, const float* noise, const int64_t* class_ids, const int64_t* neg_class_ids,
                       const double* t_list, int steps, int sample_type, int loop_kind, const float* eps, uint64_t seed, float* out, int batch,
                       void* workspace, size_t workspace_bytes, int use_graph, void* stream) {
    if (!h || !sc || !noise || !class_ids || !t_list || !out) return fail(FG_EINVAL, "null argument");
    int rc = check_sampler_args(t_list, steps, sample_type, loop_kind, sc->schedule);
    if (rc) return rc;
    if (loop_kind == FG_LOOP_MEANFLOW && (!h->cfg.r_timestep || !sc->net_pred_flow))
        return fail(FG_EINVAL, "FG_LOOP_MEANFLOW needs a flow-predicting r_timestep network");
    if (loop_kind == FG_LOOP_MEANFLOW && sc->use_sit_convention) return fail(FG_EINVAL, "FG_LOOP_MEANFLOW with use_sit_convention is not implemented");
    if (loop_kind == FG_LOOP_EULER && !sc->net_pred_flow) return fail(FG_EINVAL, "FG_LOOP_EULER needs a flow-predicting network");
    if (neg_class_ids && loop_kind != FG_LOOP_EULER) return fail(FG_EINVAL, "neg_class_ids belong to FG_LOOP_EULER (classifier-free guidance)");
    if (!(sc->t_scale > 0.0)) return fail(FG_EINVAL, "t_scale must be positive");
    DitLoopWs w;
    w.guided = neg_class_ids != nullptr;
    if ((rc = setup_ws(dit_sampler_plan, h, batch, workspace, workspace_bytes, w))) return rc;
    if (!h->packed) return fail(FG_ENOTREADY, "weights are not packed (call fg_dit_pack_weights)");
    if (h->take_error())
        return fail(FG_EINVAL, "an earlier call on this handle met a class index outside the %d rows of y_embedder.class_embeddings (its output is NaN)",
                    h->cfg.embedding_rows);
    int64_t tsb, gsb;
    memcpy(&tsb, &sc->t_scale, 8);
    memcpy(&gsb, &sc->guidance_scale, 8);
    return sampler_launch(h->sampler, batch, t_list, steps, sample_type, loop_kind, seed, w.tl, w.seed, use_graph,
                          {(int64_t)(uintptr_t)noise, (int64_t)(uintptr_t)class_ids, (int64_t)(uintptr_t)neg_class_ids, (int64_t)(uintptr_t)eps,
                           (int64_t)(uintptr_t)out, (int64_t)(uintptr_t)workspace, tsb, gsb, sc->use_sit_convention, sc->time_cond_diff,
                           sc->net_pred_flow, sc->schedule, (int64_t)h->cmode},
                          (hipStream_t)stream, [&](hipStream_t q) {
                              return dit_enqueue_sampler(h, *sc, noise, class_ids, neg_class_ids, t_list, steps, sample_type, loop_kind, eps, out,
                                                         batch, w, q);
                          });
}

}  // extern "C"

// ---- causal video DiT -------------------------------------------------------------------------------------------------------------
namespace {

struct WanLoopWs {
    float *xc, *xn, *v, *eps, *te;  // chunk buffers [B, C, f, H, W] (f <= the longest chunk) and the per-frame embedder timesteps
    double* tl;
    uint64_t* seed;
    void* net;
    size_t net_bytes;
};

size_t wan_sampler_plan(const fg_wan* h, int B, int fmax, int H, int W, Arena& A, WanLoopWs& w) {
    const size_t per = (size_t)B * h->cfg.in_channels * fmax * H * W;
    w.xc = A.get<float>(per);
    w.xn = A.get<float>(per);
    w.v = A.get<float>(per);
    w.eps = A.get<float>(per);
    w.te = A.get<float>((size_t)B * fmax);
    w.tl = A.get<double>(ScalarRing::kDoubles);
    w.seed = A.get<uint64_t>(2);
    w.net_bytes = fg_wan_workspace_bytes(h, B, fmax, H, W);
    w.net = A.take(w.net_bytes);
    return (A.off + 255) & ~(size_t)255;
}

// frames per chunk of the student loops: `chunk_size` each, the remainder of num_frames joins the FIRST chunk (causvid.py:120-128)
void wan_chunks(int frames, int chunk, std::vector<std::pair<int, int>>& out) {
    out.clear();
    const int n = frames / chunk, rem = frames % chunk;
    if (n == 0) {
        out.push_back({0, rem});
        return;
    }
    for (int i = 0; i < n; ++i) {
        const int a = i == 0 ? 0 : chunk * i + rem, b = chunk * (i + 1) + rem;
        out.push_back({a, b});
    }
}

}  // namespace

extern "C" {

size_t fg_wan_sampler_workspace_bytes(const fg_wan* h, int batch, int frames, int height, int width) {
    if (!h || !wan_shape_ok(batch, frames, height, width)) return 0;
    const int chunk = h->cfg.chunk_size, fmax = frames < chunk ? frames : chunk + frames % chunk;
    Arena A;
    A.dry = true;
    WanLoopWs w;
    return wan_sampler_plan(h, batch, fmax, height, width, A, w);
}

int fg_wan_sampler_run(fg_wan* h, const fg_wan_sampler_config* sc, float* x, const double* t_list, int steps, int sample_type, const int* exit_steps,
                       const float* eps, uint64_t seed, int batch, int frames, int height, int width, void* workspace, size_t workspace_bytes,
                       int use_graph, void* stream) {
    if (!h || !sc || !x || !t_list) return fail(FG_EINVAL, "null argument");
    int rc;
    if ((rc = wan_refuse_chunked(h, "loops")) || (rc = check_sampler_args(t_list, steps, sample_type, FG_LOOP_X0, sc->schedule))) return rc;
    if (!(sc->t_scale > 0.0)) return fail(FG_EINVAL, "t_scale must be positive");
    if (!wan_shape_ok(batch, frames, height, width) || frames > h->cfg.total_num_frames || !workspace || (((uintptr_t)workspace) & 255))
        return fail(FG_EINVAL, "bad batch / frames (<= total_num_frames = %d) / size / workspace", h->cfg.total_num_frames);
    const int chunk = h->cfg.chunk_size, prefill = sc->prefill_frames;
    if (prefill < 0 || prefill >= frames || (prefill > 0 && ((prefill % chunk) || (frames % chunk))))
        return fail(FG_EINVAL, "prefill_frames must be in [0, frames) and, like frames then, a multiple of chunk_size = %d", chunk);
    const float cn32 = (float)sc->context_noise;  // (the reference builds t_cache as a tensor of the latents' dtype, causvid.py:174)
    if (sc->context_noise < 0.0 || (sc->context_noise > 0.0 && (double)cn32 > (sc->schedule == FG_SCHEDULE_RF ? 0.999 : 80.0)))
        return fail(FG_EINVAL, "context_noise outside the schedule's range");
    std::vector<std::pair<int, int>> chunks;
    wan_chunks(frames, chunk, chunks);
    if (exit_steps)
        for (size_t ci = 0; ci < chunks.size(); ++ci)
            if (exit_steps[ci] < 0 || exit_steps[ci] >= steps) return fail(FG_EINVAL, "exit_steps[%zu] = %d outside [0, %d)", ci, exit_steps[ci], steps);
    const int fmax = frames < chunk ? frames : chunk + frames % chunk;
    Arena A;
    A.base = (char*)workspace;
    WanLoopWs w;
    const size_t need = wan_sampler_plan(h, batch, fmax, height, width, A, w);
    if (need > workspace_bytes) return fail(FG_ENOMEM, "workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    if (!h->packed) return fail(FG_ENOTREADY, "weights are not packed (call fg_wan_pack_weights)");
    if ((rc = wan_conditions_ready(h, batch, frames, height, width))) return rc;
    hipStream_t s = (hipStream_t)stream;
    // `net.clear_caches()` of the loop's first line (causvid.py:113): nothing is stored any more.  (No memset here: this loop writes every
    // cache row before any call reads it; the clear at the end of the loop leaves the buffers zeroed for whoever calls next.  The text
    // condition stays: the caller set it for THIS call.)
    if ((rc = wan_ensure_caches(h, batch, height, width, s))) return rc;  // (allocation must not fall inside a capture)
    h->cur.stored_rows = 0;
    SamplerCache& st = h->sampler;
    if ((rc = st.ring.upload(t_list, steps + 1, seed, w.tl, w.seed, s))) return rc;
    if (h->chunk_graphs.size() < chunks.size()) h->chunk_graphs.resize(chunks.size());

    const int C = h->cfg.in_channels;
    const int64_t hw = (int64_t)height * width, rows = (int64_t)batch * C, vid_pitch = (int64_t)frames * hw;
    const int nsde = steps - 1 + (sc->context_noise > 0.0 ? 1 : 0);  // injected noise tensors per video: one per re-noising step (+ the cache call's)
    for (size_t ci = 0; ci < chunks.size(); ++ci) {
        const int f0 = chunks[ci].first, f1 = chunks[ci].second, nf = f1 - f0;
        const int64_t run = (int64_t)nf * hw, total = rows * run;
        const bool fill_only = f1 <= prefill;  // the bridged head of an extrapolated segment: cache fill at t = 0 only (causvid.py:283-300)
        const int last = exit_steps ? exit_steps[ci] : steps - 1;  // Self-Forcing: the chunk leaves at its exit step (self_forcing.py:158-200)
        auto enqueue = [&](hipStream_t q) -> int {
            int r;
            HIP_TRY(launch_copy_rows(x + f0 * hw, vid_pitch, w.xc, run, run, rows, q));
            float* cur = w.xc;   // x_cur of the step
            float* nxt = w.xn;   // x_next
            auto draw = [&](int j, const float** e) -> int {  // the j-th noise tensor of this chunk: injected slice or Philox
                if (eps) {
                    HIP_TRY(launch_copy_rows(eps + (size_t)j * rows * vid_pitch + f0 * hw, vid_pitch, w.eps, run, run, rows, q));
                } else {
                    HIP_TRY(launch_randn(w.eps, total, 0, (uint64_t)(ci * (size_t)(steps + 1) + j), w.seed, q));
                }
                *e = w.eps;
                return FG_OK;
            };
            if (!fill_only) {
                for (int i = 0; i <= last; ++i) {
                    HIP_TRY(launch_embed_times(w.tl, i, 0.0, -2, 0.0, sc->t_scale, 0, 0, 0, w.te, nullptr, batch * nf, q));
                    if ((r = wan_forward(h, cur, w.te, w.v, batch, nf, height, width, f0, 0, 0, w.net, w.net_bytes, q))) return r;
                    if (sc->net_pred_flow) HIP_TRY(launch_flow_to_x0(cur, w.v, w.tl, i, 1.0f, nxt, total, q));  // fwd_pred_type = "x0"
                    else HIP_TRY(hipMemcpyAsync(nxt, w.v, sizeof(float) * total, hipMemcpyDeviceToDevice, q));
                    if (i < last && t_list[i + 1] > 0) {  // causvid.py:150-163; an exit step's prediction is the chunk's output as it is
                        if ((r = renoise_x0(i, sample_type, sc->schedule, cur, nxt, nxt, w.eps, w.tl, total, q, draw))) return r;
                    }
                    std::swap(cur, nxt);
                }
                HIP_TRY(launch_copy_rows(cur, run, x + f0 * hw, vid_pitch, run, rows, q));  // x[:, :, start:end] = x_next
            }
            // the cache-fill call on the finished chunk at t = 0, or re-noised to context_noise (:166-185)
            const float* xcache = cur;
            if (sc->context_noise > 0.0 && !fill_only) {
                const float* e = nullptr;
                if ((r = draw(steps - 1, &e))) return r;
                HIP_TRY(launch_forward_process(cur, e, (double)cn32, nullptr, 0, sc->schedule, nxt, total, q));
                xcache = nxt;
                HIP_TRY(launch_embed_times(nullptr, -1, (double)cn32, -2, 0.0, sc->t_scale, 0, 0, 1, w.te, nullptr, batch * nf, q));
            } else {
                HIP_TRY(launch_embed_times(w.tl, steps, 0.0, -2, 0.0, sc->t_scale, 0, 0, 0, w.te, nullptr, batch * nf, q));
            }
            return wan_forward(h, xcache, w.te, w.v, batch, nf, height, width, f0, 1, 0, w.net, w.net_bytes, q);
        };
        if (!use_graph) {
            if ((rc = enqueue(s))) return rc;
            continue;
        }
        // what the chunk's launches bake in; the graph of a chunk also depends on the host-side cache bookkeeping (stored_rows), which the
        // loop leaves in the same state at this point of every call
        int64_t tsb, cnb;
        memcpy(&tsb, &sc->t_scale, 8);
        memcpy(&cnb, &sc->context_noise, 8);
        std::vector<int64_t> key = {batch, frames, height, width, steps, sample_type, last, f0, f1, fill_only, zero_mask(t_list, steps),
                                    (int64_t)(uintptr_t)x, (int64_t)(uintptr_t)eps, (int64_t)(uintptr_t)workspace, tsb, cnb, sc->net_pred_flow,
                                    sc->schedule, nsde};
        wan_graph_key_tail(h, key);
        // (capture runs the same host bookkeeping as an eager pass; a replay must apply it too)
        const int stored_before = h->cur.stored_rows;
        GraphEntry& ge = h->chunk_graphs[ci];
        const bool hit = ge.exec && ge.key == key;
        if ((rc = graph_run(ge, key, st.cap, s, enqueue))) return rc;
        if (hit) {
            const int end_rows = f1 * (height / 2) * (width / 2);
            h->cur.stored_rows = end_rows > stored_before ? end_rows : stored_before;
        }
    }
    // `net.clear_caches()` at the end of the loop (causvid.py:184): the next call starts from empty caches (and sets its text again)
    return fg_wan_clear_caches(h, s);
}

}  // extern "C" (reopened below)

// ---- causal video DiT: the guided teacher sampler -----------------------------------------------------------------------------------
namespace {

// The two guided loops' workspace: a chunk of the chunked loop (Fr = its longest chunk), the whole video of the bidirectional one
struct WanGuidedWs {
    float *xin, *v;          // the network's input [Be, C, f, H, W] (guided: the chunk twice, rows [0, B) and [B, 2 B)) and its flow
    float *xl, *mp, *eps;    // x_last, m_prev of the multistep solver and the cache call's noise (chunked loop only), [B, C, f, H, W]
    float* te;
    double* sc;              // [steps + 1 timesteps | steps x 8 solver table | seed, offset as 2 x uint64]
    void* net;
    size_t net_bytes;
};

// C: the video's channels (cfg.in_channels in the chunked loop, vch() in the bidirectional one); full: the bidirectional loop - no
// cache call, so no noise buffer, and the bidirectional call's workspace
size_t wan_guided_plan(const fg_wan* h, int B, int stack, int C, int Fr, int H, int W, int steps, bool full, Arena& A, WanGuidedWs& w) {
    const size_t per = (size_t)B * C * Fr * H * W;
    w.xin = A.get<float>(per * stack);
    w.v = A.get<float>(per * stack);
    w.xl = A.get<float>(per);
    w.mp = A.get<float>(per);
    w.eps = A.get<float>(full ? 0 : per);
    w.te = A.get<float>((size_t)B * stack * Fr);
    w.sc = A.get<double>(9 * (size_t)steps + 3);
    w.net_bytes = full ? fg_wan_full_workspace_bytes(h, B * stack, Fr, H, W) : fg_wan_workspace_bytes(h, B * stack, Fr, H, W);
    w.net = A.take(w.net_bytes);
    return (A.off + 255) & ~(size_t)255;
}

constexpr int kGuidedMaxSteps = 4096;  // a sanity bound on the table's size, not a property of the loop

// What the two guided loops ask of their step arguments before they look at the video or the handle's state
int wan_check_guided_args(const fg_wan_guided_sampler_config* sc, const double* t_list, const double* table, int steps) {
    if (steps < 1 || steps > kGuidedMaxSteps) return fail(FG_EINVAL, "steps must be in [1, %d]", kGuidedMaxSteps);
    if (!(sc->t_scale > 0.0)) return fail(FG_EINVAL, "t_scale must be positive");
    if (sc->guidance != 0 && sc->guidance != 1) return fail(FG_EINVAL, "guidance must be 0 (batch B) or 1 (stacked batch 2 B)");
    for (int i = 0; i < steps; ++i)
        if (!(t_list[i] >= 0.0 && t_list[i] <= 1.0)) return fail(FG_EINVAL, "t_list[%d] = %g outside [0, 1]", i, t_list[i]);
    for (int i = 0; i < 8 * steps; ++i)
        if (!std::isfinite(table[i])) return fail(FG_EINVAL, "table[%d][%d] is not finite", i / 8, i % 8);
    return FG_OK;
}

// The guided loops' step scalars [steps + 1 timesteps (the last 0: the cache-fill call's) | steps x 8 solver table | seed, offset] do
// not fit the scalar ring: they go up from one pinned host copy of 9 steps + 3 doubles, on the caller's stream before any graph
// launch; the copy is rewritten only after the event behind its previous upload has completed.
int wan_upload_step_scalars(fg_wan* h, const double* t_list, const double* table, int steps, uint64_t seed, double* dev, hipStream_t s) {
    const size_t nd = 9 * (size_t)steps + 3;
    if (!h->pin_ev) HIP_TRY(hipEventCreateWithFlags(&h->pin_ev, hipEventDisableTiming));
    if (h->pin_used) HIP_TRY(hipEventSynchronize(h->pin_ev));
    if (h->pin_doubles < nd) {
        if (h->pin) (void)hipHostFree(h->pin);
        h->pin = nullptr, h->pin_doubles = 0;
        HIP_TRY(hipHostMalloc((void**)&h->pin, sizeof(double) * nd));
        h->pin_doubles = nd;
    }
    for (int i = 0; i < steps; ++i) h->pin[i] = t_list[i];
    h->pin[steps] = 0.0;
    memcpy(h->pin + steps + 1, table, sizeof(double) * 8 * steps);
    const uint64_t sd[2] = {seed, 0};
    memcpy(h->pin + 9 * (size_t)steps + 1, sd, sizeof(sd));
    HIP_TRY(hipMemcpyAsync(dev, h->pin, sizeof(double) * nd, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(h->pin_ev, s));
    h->pin_used = true;
    return FG_OK;
}

}  // namespace

extern "C" {

size_t fg_wan_guided_sampler_workspace_bytes(const fg_wan* h, int batch, int frames, int height, int width, int steps, int guidance) {
    if (!h || !wan_shape_ok(batch, frames, height, width) || steps < 1 || steps > kGuidedMaxSteps) return 0;
    const int chunk = h->cfg.chunk_size, fmax = frames < chunk ? frames : chunk + frames % chunk;
    Arena A;
    A.dry = true;
    WanGuidedWs w;
    return wan_guided_plan(h, batch, guidance ? 2 : 1, h->cfg.in_channels, fmax, height, width, steps, false, A, w);
}

int fg_wan_guided_sampler_run(fg_wan* h, const fg_wan_guided_sampler_config* sc, float* x, const double* t_list, const double* table, int steps,
                              const float* eps, uint64_t seed, int batch, int frames, int height, int width, void* workspace,
                              size_t workspace_bytes, int use_graph, void* stream) {
    if (!h || !sc || !x || !t_list || !table) return fail(FG_EINVAL, "null argument");
    int rc;
    if ((rc = wan_refuse_chunked(h, "loops")) || (rc = wan_check_guided_args(sc, t_list, table, steps))) return rc;
    if (!wan_shape_ok(batch, frames, height, width) || frames > h->cfg.total_num_frames || !workspace || (((uintptr_t)workspace) & 255))
        return fail(FG_EINVAL, "bad batch / frames (<= total_num_frames = %d) / size / workspace", h->cfg.total_num_frames);
    const float cn32 = (float)sc->context_noise;  // (t_cache is a tensor of the latents' dtype, network_causal.py:1268)
    if (!(sc->context_noise >= 0.0) || (double)cn32 > 0.999) return fail(FG_EINVAL, "context_noise outside [0, 0.999]");
    if (h->tag != 0) return fail(FG_EINVAL, "the guided loop runs on cache tag 0 (call fg_wan_select_cache_tag(h, 0))");
    const int guided = sc->guidance, stack = guided ? 2 : 1, Be = batch * stack;
    const int chunk = h->cfg.chunk_size, fmax = frames < chunk ? frames : chunk + frames % chunk;
    std::vector<std::pair<int, int>> chunks;
    wan_chunks(frames, chunk, chunks);
    Arena A;
    A.base = (char*)workspace;
    WanGuidedWs w;
    const size_t need = wan_guided_plan(h, batch, stack, h->cfg.in_channels, fmax, height, width, steps, false, A, w);
    if (need > workspace_bytes) return fail(FG_ENOMEM, "workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    if (!h->packed) return fail(FG_ENOTREADY, "weights are not packed (call fg_wan_pack_weights)");
    if ((rc = wan_conditions_ready(h, Be, frames, height, width, guided ? " with [cond; neg_cond]" : ""))) return rc;
    hipStream_t s = (hipStream_t)stream;
    // as in fg_wan_sampler_run: `self.clear_caches()` of the loop's first lines (network_causal.py:1216) without a memset, the text stays
    if ((rc = wan_ensure_caches(h, Be, height, width, s))) return rc;  // (allocation must not fall inside a capture)
    h->cur.stored_rows = 0;
    if ((rc = wan_upload_step_scalars(h, t_list, table, steps, seed, w.sc, s))) return rc;
    const double* tl = w.sc;
    const double* tab = w.sc + steps + 1;
    const uint64_t* seed_dev = (const uint64_t*)(w.sc + 9 * (size_t)steps + 1);
    if (h->guided_graphs.size() < chunks.size()) h->guided_graphs.resize(chunks.size());

    const int C = h->cfg.in_channels;
    const int64_t hw = (int64_t)height * width, rows = (int64_t)batch * C, vid_pitch = (int64_t)frames * hw;
    for (size_t ci = 0; ci < chunks.size(); ++ci) {
        const int f0 = chunks[ci].first, f1 = chunks[ci].second, nf = f1 - f0;
        const int64_t run = (int64_t)nf * hw, total = rows * run;
        float* x2 = guided ? w.xin + total : nullptr;  // the unconditional rows of the stacked input
        auto enqueue = [&](hipStream_t q) -> int {
            int r;
            HIP_TRY(launch_copy_rows(x + f0 * hw, vid_pitch, w.xin, run, run, rows, q));
            if (x2) HIP_TRY(launch_copy_rows(x + f0 * hw, vid_pitch, x2, run, run, rows, q));
            for (int i = 0; i < steps; ++i) {
                HIP_TRY(launch_embed_times(tl, i, 0.0, -2, 0.0, sc->t_scale, 0, 0, 0, w.te, nullptr, Be * nf, q));
                if ((r = wan_forward(h, w.xin, w.te, w.v, Be, nf, height, width, f0, 0, 0, w.net, w.net_bytes, q))) return r;
                HIP_TRY(launch_guided_multistep(w.v, w.xin, x2, w.xl, w.mp, tab + 8 * (size_t)i, guided, i == 0, total, q));
            }
            HIP_TRY(launch_copy_rows(w.xin, run, x + f0 * hw, vid_pitch, run, rows, q));  // x[:, :, start:end] = x_next
            // the cache-fill call on the finished chunk at t = 0, or re-noised to context_noise (:1263-1289); both halves hold the chunk
            if (sc->context_noise > 0.0) {
                if (eps) HIP_TRY(launch_copy_rows(eps + f0 * hw, vid_pitch, w.eps, run, run, rows, q));
                else HIP_TRY(launch_randn(w.eps, total, 0, (uint64_t)ci, seed_dev, q));
                HIP_TRY(launch_forward_process(w.xin, w.eps, (double)cn32, nullptr, 0, FG_SCHEDULE_RF, w.xin, total, q));
                if (x2) HIP_TRY(hipMemcpyAsync(x2, w.xin, sizeof(float) * total, hipMemcpyDeviceToDevice, q));
                HIP_TRY(launch_embed_times(nullptr, -1, (double)cn32, -2, 0.0, sc->t_scale, 0, 0, 1, w.te, nullptr, Be * nf, q));
            } else {
                HIP_TRY(launch_embed_times(tl, steps, 0.0, -2, 0.0, sc->t_scale, 0, 0, 0, w.te, nullptr, Be * nf, q));
            }
            return wan_forward(h, w.xin, w.te, w.v, Be, nf, height, width, f0, 1, 0, w.net, w.net_bytes, q);
        };
        if (!use_graph) {
            if ((rc = enqueue(s))) return rc;
            continue;
        }
        // what the chunk's launches bake in (timesteps, table with the guidance scale, and the seed are device memory); the host-side
        // cache bookkeeping is in the same state at this point of every call
        int64_t tsb, cnb;
        memcpy(&tsb, &sc->t_scale, 8);
        memcpy(&cnb, &sc->context_noise, 8);
        std::vector<int64_t> key = {batch, guided, frames, height, width, steps, f0, f1, (int64_t)(uintptr_t)x, (int64_t)(uintptr_t)eps,
                                    (int64_t)(uintptr_t)workspace, tsb, cnb};
        wan_graph_key_tail(h, key);
        const int stored_before = h->cur.stored_rows;
        GraphEntry& ge = h->guided_graphs[ci];
        const bool hit = ge.exec && ge.key == key;
        if ((rc = graph_run(ge, key, h->sampler.cap, s, enqueue))) return rc;
        if (hit) {  // (capture runs the same host bookkeeping as an eager pass; a replay must apply it too)
            const int end_rows = f1 * (height / 2) * (width / 2);
            h->cur.stored_rows = end_rows > stored_before ? end_rows : stored_before;
        }
    }
    return fg_wan_clear_caches(h, s);  // `self.clear_caches()` after the last chunk (:1292)
}

}  // extern "C" (reopened below)

// ---- bidirectional video DiT: the whole-video loops around fg_wan_forward_full ------------------------------------------------------
//   fg_wan_full_sampler_run         FastGenModel._student_sample_loop (methods/model.py:315-372) and MeanFlowModel._student_sample_loop
//                                   (consistency_model/mean_flow.py:336-381): dit_enqueue_sampler's structure with per-frame embedder rows
//   fg_wan_full_guided_sampler_run  Wan.sample (Wan/network.py:919-988): the guided multistep loop over the whole video
// No self-attention cache is allocated, read or moved; the text is the selected tag's (fg_wan_set_text).
namespace {

struct WanFullLoopWs {
    float *x, *v, *pred, *eps, *te, *re;
    double* tl;
    uint64_t* seed;
    void* net;
    size_t net_bytes;
};

size_t wan_full_sampler_plan(const fg_wan* h, int B, int Fr, int H, int W, Arena& A, WanFullLoopWs& w) {
    const size_t per = (size_t)B * h->vch() * Fr * H * W;  // (the video's channels: the latents alone on an image-to-video handle)
    w.x = A.get<float>(per);
    w.v = A.get<float>(per);
    w.pred = A.get<float>(per);
    w.eps = A.get<float>(per);
    w.te = A.get<float>((size_t)B * Fr);
    w.re = A.get<float>((size_t)B * Fr);
    w.tl = A.get<double>(ScalarRing::kDoubles);
    w.seed = A.get<uint64_t>(2);
    w.net_bytes = fg_wan_full_workspace_bytes(h, B, Fr, H, W);
    w.net = A.take(w.net_bytes);
    return (A.off + 255) & ~(size_t)255;
}

bool wan_full_shape_ok(const fg_wan* h, int batch, int frames, int height, int width) {
    return h && wan_shape_ok(batch, frames, height, width) && frames <= h->cfg.rope_max_seq_len;
}

}  // namespace

extern "C" {

size_t fg_wan_full_sampler_workspace_bytes(const fg_wan* h, int batch, int frames, int height, int width) {
    if (!wan_full_shape_ok(h, batch, frames, height, width)) return 0;
    Arena A;
    A.dry = true;
    WanFullLoopWs w;
    return wan_full_sampler_plan(h, batch, frames, height, width, A, w);
}

int fg_wan_full_sampler_run(fg_wan* h, const fg_wan_sampler_config* sc, const float* noise, const double* t_list, int steps, int sample_type,
                            int loop_kind, const float* eps, uint64_t seed, float* out, int batch, int frames, int height, int width,
                            void* workspace, size_t workspace_bytes, int use_graph, void* stream) {
    if (!h || !sc || !noise || !t_list || !out) return fail(FG_EINVAL, "null argument");
    int rc = check_sampler_args(t_list, steps, sample_type, loop_kind, sc->schedule);
    if (rc) return rc;
    if (loop_kind == FG_LOOP_EULER) return fail(FG_EINVAL, "FG_LOOP_EULER is not a loop of this network (fg_wan_full_guided_sampler_run)");
    if (loop_kind == FG_LOOP_MEANFLOW && (!h->ext.r_timestep || !sc->net_pred_flow))
        return fail(FG_EINVAL, "FG_LOOP_MEANFLOW needs a flow-predicting network with the r_embedder (fg_wan_create_ex, r_timestep = 1)");
    if (loop_kind == FG_LOOP_MEANFLOW && h->is_ti2v)
        return fail(FG_EINVAL, "FG_LOOP_MEANFLOW is not implemented for a first-frame-replacement handle (the reference writes the first-frame "
                    "latents into the velocity there)");
    if (!(sc->t_scale > 0.0)) return fail(FG_EINVAL, "t_scale must be positive");
    if (sc->context_noise != 0.0 || sc->prefill_frames != 0) return fail(FG_EINVAL, "context_noise and prefill_frames must be 0: there is no cache to fill");
    if (!wan_full_shape_ok(h, batch, frames, height, width) || !workspace || (((uintptr_t)workspace) & 255))
        return fail(FG_EINVAL, "bad batch / frames (<= rope_max_seq_len = %d) / size / workspace", h->cfg.rope_max_seq_len);
    Arena A;
    A.base = (char*)workspace;
    WanFullLoopWs w;
    const size_t need = wan_full_sampler_plan(h, batch, frames, height, width, A, w);
    if (need > workspace_bytes) return fail(FG_ENOMEM, "workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    if (!h->packed) return fail(FG_ENOTREADY, "weights are not packed (call fg_wan_pack_weights)");
    if ((rc = wan_conditions_ready(h, batch, frames, height, width))) return rc;
    const int rows = batch * frames;
    const int64_t total = (int64_t)batch * h->vch() * frames * height * width, hw1 = (int64_t)height * width;
    auto enqueue = [&](hipStream_t q) -> int {
        // the network on w.x at t_i into v; ri: MeanFlow's r (-1: 0, else t_list[ri]), -2: none.  The rows carry r itself: the call
        // forms t - r for time_cond_diff
        auto net = [&](int i, int ri, float* v) -> int {
            HIP_TRY(launch_embed_times(w.tl, i, 0.0, ri, 0.0, sc->t_scale, 0, 0, 0, w.te, w.re, rows, q));
            const WanFull full{ri == -2 ? nullptr : w.re, nullptr, 0};
            return wan_forward(h, w.x, w.te, v, batch, frames, height, width, 0, 0, 2, w.net, w.net_bytes, q, nullptr, &full);
        };
        const StudentLoop L{noise, t_list, steps, sample_type, sc->schedule, total, w.x, w.eps, eps, w.tl, w.seed, out, q};
        if (loop_kind == FG_LOOP_X0)
            return x0_loop(L, w.pred, [&](int i, float* pred) -> int {
                const int r = net(i, -2, w.v);
                if (r) return r;
                if (sc->net_pred_flow) HIP_TRY(launch_flow_to_x0(w.x, w.v, w.tl, i, 1.0f, pred, total, q));
                else HIP_TRY(hipMemcpyAsync(pred, w.v, sizeof(float) * total, hipMemcpyDeviceToDevice, q));
                // first-frame replacement: the conversion ran on the loop's own (unreplaced) state, as the reference converts on the
                // caller's x_t; the condition lands last (WanI2V/network.py:506-510).  The state's frame 0 is never restored between
                // steps (`preserve_conditioning`): the network reads the condition in its place and every prediction carries it.
                if (h->is_ti2v) HIP_TRY(launch_copy_rows(h->ff0, hw1, pred, (int64_t)frames * hw1, hw1, (int64_t)batch * h->vch(), q));
                return FG_OK;
            });
        return meanflow_loop(L, w.v, [&](int i, float* u) { return net(i, sample_type == FG_SAMPLE_SDE ? -1 : i + 1, u); });
    };
    int64_t tsb;
    memcpy(&tsb, &sc->t_scale, 8);
    // everything the capture bakes in: the call's shapes, buffers and settings, then what the handle owns
    std::vector<int64_t> more = {frames, height, width, (int64_t)(uintptr_t)noise, (int64_t)(uintptr_t)eps, (int64_t)(uintptr_t)out,
                                 (int64_t)(uintptr_t)workspace, tsb, sc->net_pred_flow, sc->schedule};
    wan_graph_key_tail(h, more);
    return sampler_launch(h->sampler, batch, t_list, steps, sample_type, loop_kind, seed, w.tl, w.seed, use_graph, more, (hipStream_t)stream, enqueue);
}

size_t fg_wan_full_guided_sampler_workspace_bytes(const fg_wan* h, int batch, int frames, int height, int width, int steps, int guidance) {
    if (!wan_full_shape_ok(h, batch, frames, height, width) || steps < 1 || steps > kGuidedMaxSteps) return 0;
    Arena A;
    A.dry = true;
    WanGuidedWs w;
    return wan_guided_plan(h, batch, guidance ? 2 : 1, h->vch(), frames, height, width, steps, true, A, w);
}

int fg_wan_full_guided_sampler_run(fg_wan* h, const fg_wan_guided_sampler_config* sc, float* x, const double* t_list, const double* table,
                                   int steps, int batch, int frames, int height, int width, void* workspace, size_t workspace_bytes,
                                   int use_graph, void* stream) {
    if (!h || !sc || !x || !t_list || !table) return fail(FG_EINVAL, "null argument");
    int rc;
    if ((rc = wan_check_guided_args(sc, t_list, table, steps))) return rc;
    if (sc->context_noise != 0.0) return fail(FG_EINVAL, "context_noise must be 0: there is no cache to fill");
    if (!wan_full_shape_ok(h, batch, frames, height, width) || !workspace || (((uintptr_t)workspace) & 255))
        return fail(FG_EINVAL, "bad batch / frames (<= rope_max_seq_len = %d) / size / workspace", h->cfg.rope_max_seq_len);
    const int guided = sc->guidance, stack = guided ? 2 : 1, Be = batch * stack;
    Arena A;
    A.base = (char*)workspace;
    WanGuidedWs w;
    const size_t need = wan_guided_plan(h, batch, stack, h->vch(), frames, height, width, steps, true, A, w);
    if (need > workspace_bytes) return fail(FG_ENOMEM, "workspace too small: need %zu bytes, got %zu", need, workspace_bytes);
    if (!h->packed) return fail(FG_ENOTREADY, "weights are not packed (call fg_wan_pack_weights)");
    if ((rc = wan_conditions_ready(h, Be, frames, height, width, guided ? " with [cond; neg_cond]" : ""))) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = wan_upload_step_scalars(h, t_list, table, steps, 0, w.sc, s))) return rc;  // (no draw in this loop: the seed slot goes unread)
    const double* tl = w.sc;
    const double* tab = w.sc + steps + 1;
    const int64_t total = (int64_t)batch * h->vch() * frames * height * width;
    float* x2 = guided ? w.xin + total : nullptr;  // the unconditional rows of the stacked input
    auto enqueue = [&](hipStream_t q) -> int {
        HIP_TRY(hipMemcpyAsync(w.xin, x, sizeof(float) * total, hipMemcpyDeviceToDevice, q));
        if (x2) HIP_TRY(hipMemcpyAsync(x2, x, sizeof(float) * total, hipMemcpyDeviceToDevice, q));
        const WanFull full{nullptr, nullptr, 0};
        for (int i = 0; i < steps; ++i) {
            HIP_TRY(launch_embed_times(tl, i, 0.0, -2, 0.0, sc->t_scale, 0, 0, 0, w.te, nullptr, Be * frames, q));
            const int r = wan_forward(h, w.xin, w.te, w.v, Be, frames, height, width, 0, 0, 2, w.net, w.net_bytes, q, nullptr, &full);
            if (r) return r;
            HIP_TRY(launch_guided_multistep(w.v, w.xin, x2, w.xl, w.mp, tab + 8 * (size_t)i, guided, i == 0, total, q));
            if (h->is_ti2v) {
                // `latents[:, :, 0] = first_frame_cond[:, :, 0]` after every solver step (WanI2V/network.py:414-417): the conditional
                // rows' first frame into x and into the stacked copy, as the reference restores the one latent tensor both calls read.
                // Its zeroing of the guided flow on frame 0 (:406-410) is unobservable here: the solver step is elementwise, so frame 0
                // of the flow reaches frame 0 of x, x_last and m_prev only, x's is overwritten right here, and the other two are read
                // for frame 0 of later steps alone.
                const int64_t hw1 = (int64_t)height * width, planes = (int64_t)batch * h->vch();
                HIP_TRY(launch_copy_rows(h->ff0, hw1, w.xin, (int64_t)frames * hw1, hw1, planes, q));
                if (x2) HIP_TRY(launch_copy_rows(h->ff0, hw1, x2, (int64_t)frames * hw1, hw1, planes, q));
            }
        }
        HIP_TRY(hipMemcpyAsync(x, w.xin, sizeof(float) * total, hipMemcpyDeviceToDevice, q));
        return FG_OK;
    };
    if (!use_graph) return enqueue(s);
    // what the launches bake in (timesteps and the table with the guidance scale are device memory)
    int64_t tsb;
    memcpy(&tsb, &sc->t_scale, 8);
    std::vector<int64_t> key = {batch, guided, frames, height, width, steps, (int64_t)(uintptr_t)x, (int64_t)(uintptr_t)workspace, tsb};
    wan_graph_key_tail(h, key);
    return graph_run(h->full_guided_graph, key, h->sampler.cap, s, enqueue);
}
