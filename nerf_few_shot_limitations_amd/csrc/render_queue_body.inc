// render_queue_body.inc -- the march of render_queue_kernel and render_queue_occ_kernel (fused_impl.hpp), included inside each of them.
// In scope: the template parameters Net, Mode, NT, WAVES, LP, LD; `constexpr bool OCC`; `P` (RenderKArgs: in the plain kernel the kernel
// argument itself) and `G` (OccDev, read under OCC only).  Shared as text, not as an inline function: behind a reference to its
// arguments the plain kernel compiles to other instructions than it had, and its code is to stay what it was.
    static_assert(NT == 1 || NT == 2, "a wave marches 32 or 64 sample columns");
    constexpr int STRIP = kStrip * NT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    NRF_LDS char* lds = (NRF_LDS char*)smem;
    NRF_LDS float* bias = (NRF_LDS float*)(lds + kLdsRing);
    NRF_LDS int* flags = (NRF_LDS int*)(bias + kBiasMaxFloats);
    NRF_LDS float* zl = (NRF_LDS float*)(flags + 16);
    // Per-lane ray state lives in LDS ([field][thread]: lane-linear, conflict-free) and is only pulled into registers
    // around the few instructions that use it: nothing per-ray is live across the MLP, whose register budget is full
    // (a compiler spill to scratch there is a VMEM op whose wait drains the LDS-DMA weight queue).
    NRF_LDS float* st = zl + kLadderLds;                  // == lds + kLdsState
    constexpr int nthreads = WAVES * 64;
    // ONE address register for this thread's column; fields sit at immediate offsets f*nthreads*4 (< 64 KiB, the DS
    // offset field).  The empty asm keeps the compiler from folding the (> 64 KiB) region base into 14 separate
    // per-field address registers, which it then spilled to scratch -- every reload of those drained the LDS-DMA queue.
    // Everything derived from the thread id is re-derived inside each pass from an opaque copy (tid_now): loop-invariant
    // per-lane values would otherwise be hoisted, spilled at the MLP's register peak and reloaded from scratch every pass.
    int tid_now = threadIdx.x;
    NRF_LDS float* st_me = st + tid_now;
    auto ST = [&](int f) -> NRF_LDS float& { return st_me[f * nthreads]; };
    typedef typename Mode::Act Act;
    constexpr int KT0 = pe_tiles(LP);

    int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const RenderArgs& a = P.a;
    const int S = a.n_samples;
    static_assert(WAVES * 64 <= kRenderThreads, "state rows are sized for 4 waves");
    {   // the depth ladder in LDS: the caller's table or the in-kernel formula, once per sample index (render_kernel)
        const DepthLadder lad = make_ladder(a.near, a.far, S, a.lindisp, nullptr);
        for (int i = threadIdx.x; i < S; i += blockDim.x) zl[i] = a.z_ladder ? a.z_ladder[i] : ladder_z(lad, i);
    }
    ST(F_OX) = 0.f; ST(F_OY) = 0.f; ST(F_OZ) = 0.f; ST(F_DX) = 0.f; ST(F_DY) = 0.f; ST(F_DZ) = -1.f; ST(F_Z) = 1.f;
    load_bias_table(bias, P.net.bias, P.net.n_bias);      // ends with __syncthreads()

    Pipe<WAVES, pinned_walk<Mode, NT>()> pipe;     // a wave that has run dry keeps computing (on stale inputs, storing nothing): the workgroup moves in lockstep anyway, and the skip paths cost registers in every layer
    pipe.init(P.net.stream, P.net.n_chunks, lds);
    pipe.start();

    auto z_base = [&](int s) -> float { return zl[s]; };
    auto z_of = [&](int64_t ray, int s) -> float {
        if (a.z_in) return a.z_in[ray * S + s];
        if (!a.perturb) return z_base(s);
        float u;
        if (a.t_rand) {
            u = a.t_rand[ray * S + s];
        } else {
            int ci;
            const int64_t g = global_ray(a, ray, ci);
            u = counter_uniform(a.seed + (uint64_t)ci * 0x51ED27ull, (uint64_t)g, (uint32_t)s);
        }
        const float zc = z_base(s);
        const float lower = s > 0 ? __fmul_rn(0.5f, __fadd_rn(zc, z_base(s - 1))) : zc;
        const float upper = s < S - 1 ? __fmul_rn(0.5f, __fadd_rn(z_base(s + 1), zc)) : zc;
        return __fadd_rn(lower, __fmul_rn(__fsub_rn(upper, lower), u));
    };

    // registers: only the ray id and its sample index (NT == 1: identical in both lanes of a pair)
    int ray = -1;
    int s = 0;
    // wave-uniform queue state
    int64_t pool_next = 0, pool_end = 0;
    bool exhausted = false;
    // OCC: the wave's statistics, wave-uniform (ballot counts), added to G.stats once at the end
    unsigned long long n_eval = 0, n_live = 0;

    // OCC: the first sample >= s_from of this lane's ray rr (origin / direction in its state rows) that has to be evaluated, or S;
    // the samples stepped over get weight 0 and their depth.  z: the depth of the sample returned.  A lane-divergent loop of one
    // 4-byte load (the bit field is L2-resident) and a handful of VALU instructions per sample, outside the network walk.
    auto skip_empty = [&](int64_t rr, int s_from, bool stores, float& z) -> int {
        const float o[3] = {ST(F_OX), ST(F_OY), ST(F_OZ)}, d[3] = {ST(F_DX), ST(F_DY), ST(F_DZ)};
        int s2 = s_from;
        for (; s2 < S; ++s2) {
            z = z_of(rr, s2);
            const float p[3] = {point_on_ray(o[0], d[0], z), point_on_ray(o[1], d[1], z), point_on_ray(o[2], d[2], z)};
            if (!occ_skips(G, p)) break;
            if (stores) {
                if (a.weights) a.weights[rr * S + s2] = 0.0f;
                if (a.z_vals) a.z_vals[rr * S + s2] = z;
            }
        }
        return s2;
    };

    for (int pass = 0;; ++pass) {
        tid_now = threadIdx.x;
        asm volatile("" : "+v"(tid_now));
        lane = tid_now & 63; c = lane & 31; h = lane >> 5;
        st_me = st + tid_now;
        // ---- hand new rays to idle lane pairs -------------------------------------------------
        if (!pipe.skip) {
            // OCC: a ray handed out may be finished at once (all its samples empty), so the hand-out repeats until no column is idle or
            // the queue is exhausted: every round but the last hands out at least one ray.  Its conditions are ballots: scalar branches.
            for (;;) {
                const bool need = ray < 0;
                const uint64_t m = NT == 2 ? (uint64_t)__ballot(need) : (uint64_t)(__ballot(need) & 0xFFFFFFFFull);   // NT == 1: pairs are identical, the low half suffices
                const int cnt = __builtin_popcountll(m);
                if (cnt > 0 && !exhausted) {
                    if (pool_next == pool_end) {
                        unsigned long long base = 0;
                        if (lane == 0) base = atomicAdd(a.queue, (unsigned long long)STRIP);
                        base = ((unsigned long long)__builtin_amdgcn_readfirstlane((unsigned)(base >> 32)) << 32) |
                               (unsigned)__builtin_amdgcn_readfirstlane((unsigned)base);
                        if ((int64_t)base >= a.n_rays) {
                            exhausted = true;
                        } else {
                            pool_next = (int64_t)base;
                            pool_end = (int64_t)base + STRIP < a.n_rays ? (int64_t)base + STRIP : a.n_rays;
                        }
                    }
                    if (pool_next < pool_end) {
                        const int64_t idx = pool_next + __builtin_popcountll(m & ((1ull << (NT == 2 ? lane : c)) - 1ull));
                        if (need && idx < pool_end) {
                            ray = (int)idx;
                            s = 0;
                            float o[3], d[3];
                            if (a.camera_mode) {
                                int ci;
                                const int64_t g = global_ray(a, idx, ci);
                                camera_ray(a.cams[ci], g, o, d);
                            } else {
#pragma unroll
                                for (int k = 0; k < 3; ++k) { o[k] = a.rays_o[idx * 3 + k]; d[k] = a.rays_d[idx * 3 + k]; }
                            }
                            ST(F_OX) = o[0]; ST(F_OY) = o[1]; ST(F_OZ) = o[2];
                            ST(F_DX) = d[0]; ST(F_DY) = d[1]; ST(F_DZ) = d[2];
                            ST(F_NORM) = ray_norm(d);
                            if constexpr (!OCC) {
                                ST(F_Z) = z_of(idx, 0);
                            } else {
                                const bool stores = NT == 2 || h == 0;
                                float z = 0.0f;
                                s = skip_empty(idx, 0, stores, z);
                                ST(F_Z) = z;
                                if (s >= S) {                      // nothing of this ray is occupied: no network pass, the background pixel
                                    if (stores) {                  // (the epilogue on the reset state: 0 + (1 - 0) with white_bkgd, depth 0)
                                        const float bg = a.white_bkgd ? 1.0f : 0.0f;
                                        if (a.interleaved) {
                                            *(float4*)(a.rgb + idx * 4) = make_float4(bg, bg, bg, 0.0f);
                                        } else {
                                            a.rgb[idx * 3 + 0] = bg;
                                            a.rgb[idx * 3 + 1] = bg;
                                            a.rgb[idx * 3 + 2] = bg;
                                            a.depth[idx] = 0.0f;
                                        }
                                    }
                                    ray = -1;
                                }
                            }
                            ST(F_T) = 1.0f; ST(F_R) = 0.0f; ST(F_G) = 0.0f; ST(F_B) = 0.0f; ST(F_DEPTH) = 0.0f; ST(F_ACC) = 0.0f;
                        }
                        pool_next = pool_next + cnt < pool_end ? pool_next + cnt : pool_end;
                    }
                }
                if (!OCC || cnt == 0 || exhausted) break;
            }
            // nothing left to do for this wave: keep the stream protocol, skip the math
            const int run_dry = (exhausted && pool_next == pool_end && !__any(ray >= 0)) ? 1 : 0;
            pipe.skip = (uint32_t)__builtin_amdgcn_readfirstlane(run_dry);     // provably wave-uniform: scalar branches only
            if constexpr (OCC) {
                if (G.stats && !pipe.skip) {
                    const uint64_t live = NT == 2 ? (uint64_t)__ballot(ray >= 0) : (uint64_t)(__ballot(ray >= 0) & 0xFFFFFFFFull);
                    n_eval += (unsigned)__builtin_popcountll(live);
                    n_live += 1;
                }
            }
        }

        // ---- one sample per live ray ----------------------------------------------------------
        // the state rows of column q = c + 32 n of this wave (NT == 1: the lane's own)
        auto SQ = [&](int n, int f) -> NRF_LDS float& { return (NT == 1 ? st_me : st_me - lane + c + 32 * n)[f * nthreads]; };
        auto dirT = [&](Act (&dt)[1][NT]) {
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const float d[3] = {SQ(n, F_DX), SQ(n, F_DY), SQ(n, F_DZ)};
                Act t1[pe_tiles(LD)];
                encode3<Mode, LD>(d, h, t1);
                dt[0][n] = t1[0];
            }
        };
        DinoHeld<Mode, Net::kDino ? Net::KT0 - KT0 : 1> held[NT];        // render_kernel: the gathered channels are held across NetV3's first fusion pass
        auto inputs = [&](const float (&w0)[NT], const float (&w1)[NT], Act (&x)[Net::KT0][NT], auto pass_) {
            // (a wave that has run dry encodes its stale -- valid -- state like any other: an early return here made every operand
            // tile and the held channels values merged across a branch, 300 spilled registers in the V3 build)
            constexpr int PASS = decltype(pass_)::value;
#pragma unroll
            for (int n = 0; n < NT; ++n) {
                const float zc = SQ(n, F_Z);
                float p[3];
                p[0] = point_on_ray(SQ(n, F_OX), SQ(n, F_DX), zc);
                p[1] = point_on_ray(SQ(n, F_OY), SQ(n, F_DY), zc);
                p[2] = point_on_ray(SQ(n, F_OZ), SQ(n, F_DZ), zc);
                DinoTaps tp;
                DinoRaw<Net::kDino ? Net::KT0 - KT0 : 1> raw;
                if constexpr (Net::kDino && PASS == 0) {          // the gather starts before the encoding and is blended behind it (render_kernel)
                    tp = dino_taps(a.dino, p);
                    raw.issue(a.dino.features, tp, h);
                }
                Act e1[KT0];
                encode3<Mode, LP>(p, h, e1, w0[n]);
#pragma unroll
                for (int t = 0; t < KT0; ++t) x[t][n] = e1[t];
                if constexpr (Net::kDino) {
                    constexpr int DT = Net::KT0 - KT0;
                    if constexpr (PASS == 0) held[n].finish(raw, tp);
                    Act dt[DT];
                    held[n].template tiles<PASS>(w1[n], dt);
#pragma unroll
                    for (int t = 0; t < DT; ++t) x[KT0 + t][n] = dt[t];
                }
            }
        };
        float out4[NT][4];
        Net::eval(pipe, bias, h, P.net.n_layers, inputs, dirT, out4);

        if (!pipe.skip && ray >= 0) {
            const bool last = (s + 1 == S);
            const float zc = ST(F_Z);
            const float norm = ST(F_NORM);
            const float zn = last ? 0.0f : z_of(ray, s + 1);
            const float dist = last ? __fmul_rn(1e10f, norm) : __fmul_rn(__fsub_rn(zn, zc), norm);
            Composite comp;
            comp.T = ST(F_T); comp.r = ST(F_R); comp.g = ST(F_G); comp.b = ST(F_B); comp.depth = ST(F_DEPTH); comp.acc = ST(F_ACC);
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = NT == 2 ? pick_reg(out4[0][k], out4[NT - 1][k], h != 0) : out4[0][k];
            const float w = comp.template add<Mode::FAST_EXP>(v[3], sigmoid_sel<Mode::FAST_EXP>(v[0]),
                                                              sigmoid_sel<Mode::FAST_EXP>(v[1]), sigmoid_sel<Mode::FAST_EXP>(v[2]), zc, dist);
            const int64_t rr = ray;
            const bool stores = NT == 2 || h == 0;
            if (stores) {
                if (a.weights) a.weights[rr * S + s] = w;
                if (a.z_vals) a.z_vals[rr * S + s] = zc;
            }
            bool fin = last || comp.T < a.ert_eps;
            int s_next = s + 1;
            float z_next = zn;
            if constexpr (OCC) {
                // step over the empty samples behind this one (the dist of the sample just composited went to ITS next sample, zn); a
                // ray whose rest is empty is finished here: alpha = 0 up to and including the last sample
                if (!fin) {
                    s_next = skip_empty(rr, s + 1, stores, z_next);
                    fin = s_next >= S;
                }
            }
            if (fin) {
                if (stores) {
                    // samples skipped by early termination carry weight < ert_eps: report 0 and their depths
                    for (int s2 = s_next; s2 < S; ++s2) {
                        if (a.weights) a.weights[rr * S + s2] = 0.0f;
                        if (a.z_vals) a.z_vals[rr * S + s2] = z_of(rr, s2);
                    }
                    float r = comp.r, g = comp.g, b = comp.b;
                    if (a.white_bkgd) {
                        const float bg = __fsub_rn(1.0f, comp.acc);
                        r = __fadd_rn(r, bg); g = __fadd_rn(g, bg); b = __fadd_rn(b, bg);
                    }
                    if (a.interleaved) {
                        *(float4*)(a.rgb + rr * 4) = make_float4(r, g, b, comp.depth);
                    } else {
                        a.rgb[rr * 3 + 0] = r;
                        a.rgb[rr * 3 + 1] = g;
                        a.rgb[rr * 3 + 2] = b;
                        a.depth[rr] = comp.depth;
                    }
                }
                ray = -1;
            } else {
                ST(F_T) = comp.T; ST(F_R) = comp.r; ST(F_G) = comp.g; ST(F_B) = comp.b; ST(F_DEPTH) = comp.depth; ST(F_ACC) = comp.acc;
                ST(F_Z) = z_next;
                s = s_next;
            }
        }

        // ---- workgroup-wide vote every fourth pass: leave once every wave has run dry -----------
        if ((pass & 3) == 3) {
            if (lane == 0) flags[((pass >> 2) & 1) * WAVES + wave] = (int)pipe.skip;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            const NRF_LDS int* fl = flags + ((pass >> 2) & 1) * WAVES;
            int all_done = 1;
#pragma unroll
            for (int wv = 0; wv < WAVES; ++wv) all_done &= fl[wv];
            if (all_done) break;
        }
    }
    if constexpr (OCC) {
        if (G.stats && lane == 0) {
            atomicAdd(G.stats, n_eval);
            atomicAdd(G.stats + 1, n_live);
        }
    }
    pipe.drain();
