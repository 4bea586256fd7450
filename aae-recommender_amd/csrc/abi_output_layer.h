// The step, part 2: the decoder's output layer + BCE + its backward (aae.py:176-177, 693-706) in output_form()'s four forms (abi_chains.h).
// (one of the parts of aae_abi.hip's translation unit: included there in order, not on its own)
#pragma once

namespace {

// One step's view of the fused output layer: what every launch below shares
struct DecLaunch {
    DecFusedArgs fa;            // arguments of a launch over the whole batch (fill_dec_args)
    int nblk, Bb;               // row blocks (one launch covers at most 112 rows) and rows per block (the last may be shorter)
    int ntiles, grid;           // 32-item tiles of the layer; workgroups of a launch on the whole chip
    bool win;                   // dec.lin3 beyond 2^31 bytes: the kernels' moving-window instantiations (dec_fused.h)
    DecodeMode mode;            // of the decode-backward call this launch belongs to
    bool want_ts, ts_obk;       // debug (AAE_DEC_TS): phase timeline of one tile / of dec_opt_blocks_x3_kernel ("obk")
};
unsigned long long* dec_ts_dev = nullptr;      // debug (AAE_DEC_TS): the kernels' 128 timestamps

DecFusedArgs fill_dec_args(const aae_model* m, int B, int nblk, float gscale) {
    DecFusedArgs fa;
    fa.dh2 = m->dh2.p; fa.ldh = m->ldh;
    fa.V3a = m->P[P_V3].p; fa.M = m->M[0][P_V3].p; fa.V = m->V[0][P_V3].p; fa.ldv = m->ldh;
    fa.gradV3 = m->cfg.grad_mode == AAE_GRAD_EXPORT ? m->Gr[P_V3].p : nullptr;
    fa.N = m->N; fa.B = B; fa.h = m->h; fa.gscale = gscale;
    fa.te.start = m->tstart; fa.te.eb = m->teb; fa.te.en = m->ten; fa.te.ev = m->tev;
    fa.slabs = m->slabs.p; fa.slab_stride = (size_t)(nblk > 1 ? B : std::min(m->R, 16 * kMB)) * m->ldh; fa.ld_slab = m->ldh;
    fa.partials = m->bce_partials; fa.sc = m->sc + O_DEC;
    fa.erow0 = 0; fa.dh2f = nullptr; fa.nblk = 1; fa.Bb = B;
    fa.one_term = m->bf16 ? 1 : 0; fa.dbg_skip = m->opt.dec_skip;
    fa.ts = nullptr; fa.Gt = m->Gt;
    return fa;
}

int no_kernel(const char* family) { return fail(AAE_ESTATE, std::string(family) + ": no instantiation is compiled for this hidden width and mode"); }

// ---- debug reports (AAE_DEC_TS), out of the step's path.  obk: dec_opt_blocks_x3_kernel<13, true>'s, at its launch on stream s;
// quiet: that one has been printed
int print_dec_timeline(aae_model* m, bool obk, bool quiet, hipStream_t s) {
    unsigned long long t[128];
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipMemcpy(t, dec_ts_dev, sizeof(t), hipMemcpyDeviceToHost));
    if (quiet) return AAE_OK;
    if (obk) {
        for (int w = 0; w < 2; ++w) {
            fprintf(stderr, "[dec_opt_blocks_x3 wave %d, steps 8..15, us: products | split | to the next barrier;  spare wave: - | split | requests | wait for the slot | to the next barrier]", w ? 12 : 0);
            for (int q = 0; q < 8; ++q) {
                const unsigned long long* u = t + 64 * w + 4 * q;
                if (w == 0) fprintf(stderr, "  %.2f %.2f %.2f", (u[1] - u[0]) * 0.01, (u[2] - u[1]) * 0.01, q < 7 ? ((double)u[4] - (double)u[2]) * 0.01 : 0.0);
                else fprintf(stderr, "  %.2f %.2f %.2f %.2f", (u[1] - u[0]) * 0.01, (u[2] - u[1]) * 0.01, (u[3] - u[2]) * 0.01, q < 7 ? ((double)u[4] - (double)u[3]) * 0.01 : 0.0);
            }
            fprintf(stderr, "\n");
        }
        for (int k = 0; k < 2; ++k) {
            const unsigned long long* u = t + (k ? 96 : 32);
            fprintf(stderr, "[dec_opt_blocks_x3 step %d: every wave's arrival at the step's closing barrier, us after wave 0 finished its products]", k ? 12 : 9);
            for (int w = 0; w < 16; ++w) fprintf(stderr, " %.2f", ((double)u[w] - (double)u[16]) * 0.01);
            fprintf(stderr, "\n");
        }
        return AAE_OK;
    }
    if (m->last_out_split) {
        fprintf(stderr, "[dec_crit_x3 tile 5] barrier=%.2f S0=%.2f GEMM1=%.2f BCE=%.2f GEMM3=%.2f | wg 0: prologue=%.2f loop=%.2f (%llu tiles, %.2f each) epilogue=%.2f us\n",
                (t[14] - t[0]) * 0.01, (t[1] - t[14]) * 0.01, (t[2] - t[1]) * 0.01, (t[3] - t[2]) * 0.01, (t[4] - t[3]) * 0.01,
                (t[11] - t[10]) * 0.01, (t[7] - t[11]) * 0.01, t[13], (t[7] - t[11]) * 0.01 / (double)(t[13] ? t[13] : 1),
                (t[12] - t[7]) * 0.01);
        return AAE_OK;
    }
    if (m->bf16)
        for (int k = 0; k < 5; ++k) {
            fprintf(stderr, "[dec_fused_bf16 arrivals at barrier %d, us after the unit's start]", k);
            for (int w = 0; w < 16; ++w) fprintf(stderr, " %.2f", ((double)t[16 + 16 * k + w] - (double)t[0]) * 0.01);
            fprintf(stderr, "\n");
        }
    fprintf(stderr, "[dec_fused tile 5] S0=%.2f GEMM1+BCE0=%.2f entries=%.2f GEMM2+GEMM3=%.2f S5=%.2f | tile=%.2f us, %.0f shader clocks -> %.2f GHz\n",
            (t[1] - t[0]) * 0.01, (t[2] - t[1]) * 0.01, (t[3] - t[2]) * 0.01, (t[4] - t[3]) * 0.01,
            (t[6] - t[4]) * 0.01, (t[6] - t[0]) * 0.01, (double)(t[9] - t[8]),
            (double)(t[9] - t[8]) / ((t[6] - t[0]) * 10.0));
    if (m->bf16) fprintf(stderr, "[dec_fused_bf16 S0] barrier A=%.2f work=%.2f barrier B=%.2f us\n", (t[14] - t[0]) * 0.01, (t[15] - t[14]) * 0.01, (t[1] - t[15]) * 0.01);
    fprintf(stderr, "[dec_fused wg 0] prologue=%.2f loop=%.2f (%llu tiles, %.2f each) epilogue=%.2f us\n",
            (t[11] - t[10]) * 0.01, (t[7] - t[11]) * 0.01, t[13], (t[7] - t[11]) * 0.01 / (double)(t[13] ? t[13] : 1),
            (t[12] - t[7]) * 0.01);
    return AAE_OK;
}

// ---- split forms, the critical launch (dec_crit_x3_kernel): ONE launch for all row blocks - workgroup w works on block
// w % nblk with its block of dh2 in LDS and takes every (grid / nblk)-th tile; 8 launches of 1.5 tile rounds each (-> 2, plus
// an 84 KB prologue per workgroup and launch) cost 8 x 26.5 us on a 12.5 k-item slice, one launch of 12.2 rounds what the
// 100-row step's critical launch costs.
// late join (abi_model.h): the kernel sets the deferred launch's dh2 and step scalars aside.
int launch_output_critical(aae_model* m, const DecLaunch& L, bool late, int grid, hipStream_t s) {
    DecFusedArgs b = L.fa;
    b.nblk = L.nblk; b.Bb = L.Bb;
    if (late) { b.dh2_snap = m->dh2s.p; b.sc_snap = m->sc_snap; }
    // "this launch is done" rides on the kernel's own completion signal (a hipEventRecord behind the launch is a
    // marker packet the next kernel of the stream waits for: +30 us per step); when the launch is being timed,
    // the timing pair's stop event doubles as that event.
    hipEvent_t start = nullptr, stop = m->ev_crit;
    (void)prof_pair(m, AAE_K_DEC_CRIT, &start, &stop);
    const int nb = m->fused_nb;
    // (a bf16 handle: the one-term instantiation, one matrix instruction per product; the timeline exists for <13> three-term alone)
    const bool ts = b.ts && !m->bf16 && nb == 13;
    const DecKernel kernel = pick_dec_crit_x3(nb, ts, m->bf16, L.win && !ts);
    if (!kernel) return no_kernel("dec_crit_x3");
    hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(kNT), (uint32_t)dec_crit_x3_lds_bytes(nb), s, start, stop, 0, b);
    LAUNCHCHK("dec_crit_x3");
    HIPCHK(hipStreamWaitEvent(m->side, stop, 0));
    return AAE_OK;
}

// ---- split forms, the deferred launch on the side stream behind the rest of the step, timed as AAE_K_DEC_OPT: dec_opt_x3_kernel
// over one row block, dec_opt_blocks_x3_kernel over every row block of a batch beyond one launch (any vocabulary size)
int launch_output_deferred(aae_model* m, const DecLaunch& L, bool late) {
    const int ntiles = L.ntiles, nb = m->fused_nb, B = L.fa.B;
    DecFusedArgs b = L.fa;
    b.nblk = L.nblk; b.Bb = L.Bb;
    DecKernel kernel; const char* what; int grid; uint32_t lds; bool ts = false;
    if (L.nblk > 1) {
        hipLaunchKernelGGL(dh2_frag_kernel, dim3((B + kXCH - 1) / kXCH, m->fused_nb), dim3(128), 0, m->side, m->dh2.p, m->ldh, B,
                           reinterpret_cast<u32x4_t*>(m->dh2f.p), b.one_term);
        b.dh2f = m->dh2f.p;
        // tile groups of at most kXBT tiles, the same number (+-1 tile) for every workgroup and round
        // Workgroups: one per ~16 tiles, between half and three quarters of the CUs (tools/debug/sweep_obk_wgs*.sh, late r3,
        // ms per step): 100 k items x 512 rows 0.774 / 0.725 / 0.710 / 0.703 / 0.690 / 0.755 / 0.749 on 128 / 144 / 160 /
        // 176 / 192 / 208 / 224; x 256 rows 0.506 / 0.468 / 0.443 / 0.506 on 128 / 160 / 192 / 208; x 1024 rows 1.260 /
        // 1.245 / 1.356 on 160 / 192 / 208; 47 k items x 500 rows 0.388 / 0.372 / 0.369 / 0.381 / 0.378 on 96 / 112 / 128 /
        // 144 / 160; an item slice of 12.5 k items x 800 rows 0.382 / 0.379 / 0.400 / 0.387 ms of per-rank compute on
        // 96 / 128 / 160 / 192.  (Beyond 3/4 of the chip the step's own launches lose more than this one gains.)
        // (a slice of thousands of tiles - C5: 275 k items x 512 rows, 8 594 tiles - outlasts the step's tail by far: 7/8 of the
        //  chip there, r4: one rank's step 1.58 | 1.52 | 1.61 | 1.59 ms on 192 | 224 | 240 | 256 workgroups)
        const int wg_cap = ntiles >= 4096 ? m->n_cu * 7 / 8 : m->n_cu * 3 / 4;
        // (r5: a layer of a few hundred tiles - C4: 144 - is two or three tiles per workgroup on a sixth of the chip: 0.3549 |
        //  0.3493 | 0.3489 | 0.3486 | 0.3524 ms/step on 128 | 32 | 48 | 64 | 96 workgroups, tools/debug/c4_obk_sweep.sh)
        const int by_tiles = ntiles < 384 ? std::max(32, std::min(m->n_cu / 2, ntiles / 3))
                                          : std::max(m->n_cu / 2, std::min(wg_cap, (int)(ntiles / 16.3 / 8.0 + 0.5) * 8));
        grid = std::max(1, std::min(by_tiles, std::min(ntiles, m->n_cu)));
        const int rounds = (ntiles + grid * kXBT - 1) / (grid * kXBT);
        b.tpp = grid * rounds;
        ts = L.ts_obk && nb == 13;
        kernel = pick_dec_opt_blocks_x3(nb, ts, L.win && !ts); what = "dec_opt_blocks_x3";
        lds = (uint32_t)dec_opt_blocks_x3_lds_bytes();
    } else {
        // (the 3-term bf16 emulation of dV3 = G^T dh2, dec_crit_x3.h)
        // (one-term instantiation: 78 VGPRs - six of its waves fit a SIMD, so the step's own launches would be dealt onto
        //  its CUs and run beside its streams; its LDS claim is raised until no other workgroup of the step fits there)
        // (the three-term instantiations keep dh2's third term in a 64 KB block of LDS behind the tile: ~124 KB)
        lds = (uint32_t)dec_opt_x3_lds_bytes(!m->bf16);
        if (m->bf16) lds = std::max(lds, 150u * 1024u);
        // (late join: dec_opt_x3_kernel reads the copies the critical launch set aside)
        if (late) { b.dh2 = m->dh2s.p; b.sc = m->sc_snap; }
        grid = std::min(ntiles, std::min(m->split_wgs, m->n_cu));
        kernel = pick_dec_opt_x3(nb, m->bf16, L.win); what = "dec_opt_x3";
    }
    if (!kernel) return no_kernel(what);
    hipEvent_t start = nullptr, stop = nullptr;
    (void)prof_pair(m, AAE_K_DEC_OPT, &start, &stop);
    hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(kNT), lds, m->side, start, stop, 0, b);
    LAUNCHCHK(what);
    return ts ? print_dec_timeline(m, true, false, m->side) : AAE_OK;
}

// ---- split forms: the critical launch here, the deferred launch on the side stream
int output_layer_split(aae_model* m, const DecLaunch& L, int* n_loss_partials, int* crit_slabs, hipStream_t s) {
    if (m->opt_pending) TRY(join_deferred(m, s));   // (never: every step-opening entry point joins)
    // late join (abi_model.h): single row block
    const int nblk = L.nblk;
    const bool late = m->late_enabled && nblk == 1 && !L.want_ts &&
                      m->dh2s.p && m->sc_snap && L.fa.B <= m->dh2s.rows && L.grid >= L.fa.B;
    const int wgs = nblk > 1 ? std::max(1, m->n_cu / nblk) : L.grid;
    const int crit_grid = nblk > 1 ? wgs * nblk : L.grid;
    *n_loss_partials = crit_grid;
    *crit_slabs = wgs;
    TRY(launch_output_critical(m, L, late, crit_grid, s));
    TRY(launch_output_deferred(m, L, late));
    TRY(side_done(m, m->ev_opt));
    m->opt_pending = true;
    m->late_ok = late;
    m->last_out_split = true; m->side_ordered = true;
    // an item slice's next batch (named ahead): its distinct items and their deferred-Adam catch-up behind the
    // deferred launch on the same stream (ordered behind this step's head by ev_crit; rows of the running batch
    // are skipped there, the step's own updates bring them to the same step)
    if (L.mode.only_output_layer && m->pf_armed && m->mark2 && m->lazy) TRY(launch_prefetch(m, false));
    return AAE_OK;
}

// ---- the single launch (dec_fused.h; a bf16 handle's: dec_fused_bf16.h): logits, BCE, dV3 + dec_optim and dA2 in one persistent kernel
int launch_output_single(aae_model* m, const DecLaunch& L, hipStream_t s) {
    m->last_out_split = false; m->side_ordered = false;
    ProfScope ps(m, AAE_K_DEC_FUSED, s);
    const DecKernel kernel = m->bf16 ? pick_dec_fused_bf16(m->fused_nb) : pick_dec_fused(m->fused_nb, L.win);
    if (!kernel) return no_kernel("dec_fused");
    const size_t lds = m->bf16 ? dec_fused_bf16_lds_bytes(m->fused_nb) : dec_fused_lds_bytes(L.fa.B, m->h);
    hipLaunchKernelGGL(kernel, dim3(L.grid), dim3(m->bf16 ? kBT : kNT), lds, s, L.fa);
    return AAE_OK;
}

// 256+ slabs -> 16 partial slabs (stored behind the per-workgroup ones) -> sum + act'/dropout; the same launch reduces
// the per-workgroup loss partials.  *part: the 16 partial slabs, for a chain program to sum (m->use_chain)
int reduce_slabs(aae_model* m, const DecLaunch& L, int crit_slabs, int n_loss_partials, const DropSpec& d2, const float** part_out, hipStream_t s) {
    const int B = L.fa.B, N = m->N, h = m->h;
    const size_t slab_stride = L.fa.slab_stride;
    float* part = m->slabs.p + (size_t)304 * slab_stride;
    *part_out = part;
    const size_t n4 = (size_t)B * m->ldh / 4;
    // n slabs at src -> ny partial slabs at dst (ny == 1: their sum); loss: + the per-workgroup loss partials -> the step's loss
    auto sum_slabs = [&](const float* src, int n, float* dst, size_t dst_stride, int ny, bool loss) {
        hipLaunchKernelGGL(slab_partial_kernel, dim3((unsigned)((n4 + 255) / 256), ny), dim3(256), 0, s, src, n, slab_stride, n4, dst, dst_stride,
                           loss ? m->bce_partials : (const float*)nullptr, loss ? n_loss_partials : 0, loss ? 1.0f / ((float)B * (float)N) : 0.f, m->losses, 0);
    };
    if (L.mode.only_output_layer && crit_slabs <= 64) {
        // (row blocks in one launch: 256 / nblk slabs - one pass sums them straight into dL/d(dh2), with the loss)
        sum_slabs(m->slabs.p, crit_slabs, m->da2.p, 0, 1, true);
        LAUNCHCHK("slabs -> da2");
        return AAE_OK;
    }
    sum_slabs(m->slabs.p, crit_slabs, part, slab_stride, 16, true);
    if (L.mode.only_output_layer) {
        sum_slabs(part, 16, m->da2.p, 0, 1, false);
        LAUNCHCHK("slab_partial -> da2");
    } else if (!m->use_chain) {
        hipLaunchKernelGGL(slab_reduce_actbwd_kernel, dim3(grid1d((size_t)B * h, 64)), dim3(64), 0, s, part, 16,
                           slab_stride, B, h, m->ldh, m->dh2.p, m->ldh, m->gb0.p, m->cfg.activation, d2,
                           m->cfg.seed, m->step_ctr);
        LAUNCHCHK("slab_reduce");
    }
    return AAE_OK;
}

// ---- fused forms (form: Single, Split or Blocked), then the slab reduction
int output_layer_fused(aae_model* m, OutForm form, const DecodeMode& mode, int B, float gscale, const DropSpec& d2, const float** chain_part, size_t* chain_stride, hipStream_t s) {
    if (m->bk_pending) {            // built on the side stream while this step's forward ran (aae_first_layer_forward)
        HIPCHK(hipStreamWaitEvent(s, m->ev_bk, 0));
        m->bk_pending = false;
    }
    if (!m->buckets_valid) TRY(build_tile_buckets(m, s));   // (else: the extra workgroup of this step's first chain launch did)
    DecLaunch L;
    L.mode = mode;
    // row blocks of the fused output layer: a row block covers at most 112 rows; larger batches (cfg.blocked_output) run as
    // nblk equal row blocks of the split form
    L.nblk = form == OutForm::Blocked ? row_blocks(m) : 1; L.Bb = (B + L.nblk - 1) / L.nblk;
    L.ntiles = (m->N + kTI - 1) / kTI; L.grid = std::min(L.ntiles, m->n_cu);
    L.win = x3_big_span(m->N, m->ldh);
    L.fa = fill_dec_args(m, B, L.nblk, gscale);
    L.want_ts = m->opt.dec_ts[0] != 0;
    if (L.want_ts) {
        if (!dec_ts_dev && hipMalloc(&dec_ts_dev, 128 * sizeof(unsigned long long)) != hipSuccess) return fail(AAE_EHIP, "ts alloc");
        L.fa.ts = dec_ts_dev;
    }
    int n_loss_partials = L.grid, crit_slabs = L.grid;
    // (AAE_DEC_TS: the timeline of the single launch - or, AAE_DEC_TS=x3 / obk, of the split forms' dec_crit_x3_kernel /
    // dec_opt_blocks_x3_kernel)
    L.ts_obk = L.want_ts && strcmp(m->opt.dec_ts, "obk") == 0;
    if (form == OutForm::Single) TRY(launch_output_single(m, L, s));
    else TRY(output_layer_split(m, L, &n_loss_partials, &crit_slabs, s));
    LAUNCHCHK("dec_fused");
    if (L.want_ts) TRY(print_dec_timeline(m, false, m->last_out_split && L.ts_obk, s));
    *chain_stride = L.fa.slab_stride;
    return reduce_slabs(m, L, crit_slabs, n_loss_partials, d2, chain_part, s);
}

// ---- unfused path: three GEMMs through G = dL/dlogits [B][N]
int output_layer_unfused(aae_model* m, const DecodeMode& mode, int B, float gscale, const DropSpec& d2, hipStream_t s) {
    const int N = m->N, h = m->h;
    {
        EpiBce e; e.G = m->G.p; e.ldg = m->ldn; e.gscale = gscale; e.partials = m->bce_partials;
        {
            ProfScope ps(m, AAE_K_DEC_BCE_FWD, s);
            TRY(linear_fwd(m->dh2.p, m->ldh, B, m->P[P_V3], e, s, gmode(m)));
        }
        hipLaunchKernelGGL(bce_fixup_kernel, dim3(B, m->chunks), dim3(256), 0, s, m->bv, m->dh2.p, m->ldh, m->P[P_V3].p, m->ldh,
                           h + 1, m->G.p, m->ldn, gscale, m->fix_partials);
        LAUNCHCHK("bce_fixup");
        const int ts = m->P[P_V3].rows > 4096 ? 64 : 32;   // tile edge linear_fwd picks for this layer
        TRY(finalize_bce_loss(m, ((N + ts - 1) / ts) * ((B + ts - 1) / ts), s));
    }
    // dA2 = G * V3 (K = N items, split-K slabs), then back through act2/drop2
    {
        int splits;
        const int kps = split_k_items(m, B, &splits);
        GemmShape g{m->G.p, m->P[P_V3].p, B, h, N, m->ldn, m->ldh, kps};
        EpiSlab e; e.out = m->slabs.p; e.ld = m->ldh; e.slab_stride = (size_t)m->R * m->ldh;
        {
            ProfScope ps(m, AAE_K_DEC_DA2, s);
            (void)launch_gemm_mode<0, 0, true>(gmode(m), g, e, splits, s);
        }
        LAUNCHCHK("dA2 gemm");
        if (mode.only_output_layer) {
            const size_t n4 = (size_t)B * m->ldh / 4;
            hipLaunchKernelGGL(slab_partial_kernel, dim3((unsigned)((n4 + 255) / 256), 1), dim3(256), 0, s, m->slabs.p, splits,
                               e.slab_stride, n4, m->da2.p, (size_t)0, (const float*)nullptr, 0, 0.f, m->losses, 0);
            LAUNCHCHK("slabs -> da2");
        } else
        hipLaunchKernelGGL(slab_reduce_actbwd_kernel, dim3(grid1d((size_t)B * h)), dim3(256), 0, s, m->slabs.p, splits,
                           e.slab_stride, B, h, m->ldh, m->dh2.p, m->ldh, m->gb0.p, m->cfg.activation, d2, m->cfg.seed,
                           m->step_ctr);
        LAUNCHCHK("slab_reduce");
    }
    // dV3 = G^T * dh2 -> dec_optim on V3 (the 24 B/param streaming kernel).  Like the fused path's optimiser half
    // (section 3.2c) only the NEXT step reads its result: with the fused optimiser it goes to the handle's low-priority
    // side stream, behind the rest of the step (G and dh2 stay untouched until the next step's join).
    // (not for the item slices of the vocabulary-sharded scheme: there the background GEMM slowed the replica handle's
    // kernels by more than it saved - 0.496 -> 0.560 ms of per-rank compute at world 8, tools/vocab_rank_time.py)
    if (m->side && m->cfg.grad_mode == AAE_GRAD_FUSED && !m->bf16 && !mode.only_output_layer) {
        HIPCHK(hipEventRecord(m->ev_crit, s));
        HIPCHK(hipStreamWaitEvent(m->side, m->ev_crit, 0));
        {
            ProfScope ps(m, AAE_K_DEC_DV3_ADAM, m->side);
            TRY(linear_dw(m, m->G.p, m->ldn, B, m->dh2.p, m->ldh, P_V3, O_DEC, m->side));
        }
        TRY(side_done(m, m->ev_opt));
        m->opt_pending = true;
        m->side_ordered = true;
    } else {
        m->side_ordered = false;
        ProfScope ps(m, AAE_K_DEC_DV3_ADAM, s);
        TRY(linear_dw(m, m->G.p, m->ldn, B, m->dh2.p, m->ldh, P_V3, O_DEC, s));
    }
    return AAE_OK;
}

// ---- the VAE's hidden half (reference vae.py:111-130 and its backward), one dispatcher per half: the layer-chain programs
// (abi_chains.h chain_vae_*) where the handle has them, else - a cfg.vae_wide handle wider than a chain slot, or under NO_CHAIN -
// one launch per layer: the wide AAE's products and epilogues (abi_layers.h) around vae_layers.h's two kernels.  A backward
// dispatcher ends with the weight gradients and optimiser updates of its half.
// (any other VAE handle off the chain programs: the refusal of before, for the entry points to hand on)
inline bool vae_route(const aae_model* m) { return m->use_chain || m->vae_layers; }
int vae_route_check(const aae_model* m) {
    if (vae_route(m)) return AAE_OK;
    return fail(AAE_ESTATE, "VAE mode needs the layer-chain kernels (a handle created with cfg.vae_wide = 1 runs layer by layer without them)");
}

int launch_vae_reparam_fwd(aae_model* m, const float* cond_dev, const float* eps_dev, float* z_out, bool tail, int rows, int grow0, hipStream_t s) {
    VaeReparamFwd a;
    a.mulv = m->mulv.p; a.ldm = (int)m->mulv.ld; a.eps_in = eps_dev; a.ldi = m->c;
    a.veps = m->veps.p; a.lde = (int)m->veps.ld; a.zc = m->zc.p; a.ldzc = m->ldc; a.z_out = z_out;
    a.cond = cond_dev; a.cond_inc = m->cfg.cond_inc; a.tail = tail ? 1 : 0;
    a.rows = rows; a.c = m->c; a.cp = m->cp;
    auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    a.vec = (m->c & 3) == 0 && al16(eps_dev) && al16(z_out);
    a.vec_cond = (m->c & 3) == 0 && (a.cond_inc & 3) == 0 && al16(cond_dev);
    a.seed = m->cfg.seed; a.step_ctr = m->step_ctr; a.stream_id = 12; a.grow0 = grow0;
    ProfScope ps(m, AAE_K_VAE_REPARAM, s);
    hipLaunchKernelGGL(pick_vae_reparam_fwd(), dim3((rows + 3) / 4), dim3(256), 0, s, a);
    LAUNCHCHK("vae_reparam_fwd");
    return AAE_OK;
}
// [mu | logvar] = [fc21; fc22] eh1 -> z (and the constant condition block, the bias column: tail)
int vae_encode_layers(aae_model* m, const float* cond_dev, const float* eps_dev, float* z_out, bool tail, int rows, int grow0, hipStream_t s) {
    EpiStore e; e.out = m->mulv.p; e.ld = (int)m->mulv.ld;
    TRY(linear_fwd(m->eh1.p, m->ldh, rows, m->P[P_W3], e, s, gmode(m)));
    return launch_vae_reparam_fwd(m, cond_dev, eps_dev, z_out, tail, rows, grow0, s);
}
// dh2 = act(fc3 zc)
int vae_dec_hidden_layers(aae_model* m, int rows, hipStream_t s) {
    EpiDropAct e; e.out = m->dh2.p; e.ld = m->ldh; e.act = m->cfg.activation; memset(&e.d, 0, sizeof(e.d));      // (no dropout in the VAE)
    e.seed = m->cfg.seed; e.step_ctr = m->step_ctr;
    return linear_fwd(m->zc.p, m->ldc, rows, m->P[P_V1], e, s, gmode(m));
}
// from gb0 = dL/d(pre-activation of fc3), which both forms of the output layer leave there off the chain programs (reduce_slabs,
// output_layer_unfused): dL/d(decoder input) -> gzc (and the caller), fc3's weight gradient + optimiser
int vae_backward_dec_layers(aae_model* m, float* dzc_out, hipStream_t s) {
    const int B = m->rows, cp = m->cp;
    EpiStore ez; ez.out = m->gzc.p; ez.ld = m->ldc;
    TRY(linear_dx(m->gb0.p, m->ldh, B, m->P[P_V1], cp, ez, s, gmode(m)));
    if (dzc_out) {
        hipLaunchKernelGGL(copy2d_kernel, dim3(grid1d((size_t)B * cp)), dim3(256), 0, s, m->gzc.p, m->ldc, dzc_out, cp, B, cp, 1.0f);
        LAUNCHCHK("copy dzc");
    }
    return linear_dw(m, m->gb0.p, m->ldh, B, m->zc.p, m->ldc, P_V1, O_DEC, s);
}
// from dL/dz: (dL/dmu, dL/dlogvar) with the KL gradient and the KL sum -> [fc21; fc22] -> dL/d(a1) in gb3, their weight
// gradients + optimiser, the first layer's bias and rows (as encoder_backward ends)
int vae_backward_enc_layers(aae_model* m, const float* dz_dev, int ld_dz, hipStream_t s) {
    const int B = m->rows, h = m->h;
    {
        VaeReparamBwd a;
        a.dz = dz_dev; a.lddz = ld_dz; a.mulv = m->mulv.p; a.ldm = (int)m->mulv.ld; a.veps = m->veps.p; a.lde = (int)m->veps.ld;
        a.gmulv = m->gmulv.p; a.ldg = (int)m->gmulv.ld; a.rows = B; a.c = m->c;
        a.vec = (m->c & 3) == 0 && (ld_dz & 3) == 0 && (reinterpret_cast<uintptr_t>(dz_dev) & 15) == 0;
        a.scale = m->grad_scale; a.row_kl = m->adv_terms; a.ticket = m->kl_ticket; a.loss_out = m->losses + 1;
        ProfScope ps(m, AAE_K_VAE_REPARAM, s);
        hipLaunchKernelGGL(pick_vae_reparam_bwd(), dim3((B + 3) / 4), dim3(256), 0, s, a);
        LAUNCHCHK("vae_reparam_bwd");
    }
    EpiActBwd b; b.out = m->gb3.p; b.ld = m->ldh; b.y = m->eh1.p; b.ldy = m->ldh; b.act = m->cfg.activation; memset(&b.d, 0, sizeof(b.d));
    b.seed = m->cfg.seed; b.step_ctr = m->step_ctr;
    TRY(linear_dx(m->gmulv.p, (int)m->gmulv.ld, B, m->P[P_W3], h, b, s, gmode(m)));
    TRY(linear_dw(m, m->gmulv.p, (int)m->gmulv.ld, B, m->eh1.p, m->ldh, P_W3, O_ENC, s));
    return encoder_first_layer_update(m, m->gb3.p, O_ENC, s);      // (nothing rode in a grouped launch: colsum_adam_kernel, then the item rows)
}

// (grow0: the generator row of row 0 - chain_vae_forward)
int vae_forward(aae_model* m, const float* cond_dev, const float* eps_dev, int rows, hipStream_t s, int grow0 = 0) {
    if (m->use_chain) return chain_vae_forward(m, cond_dev, eps_dev, rows, s, grow0);
    TRY(vae_route_check(m));
    TRY(vae_encode_layers(m, cond_dev, eps_dev, nullptr, true, rows, grow0, s));
    return vae_dec_hidden_layers(m, rows, s);
}
int vae_encode(aae_model* m, const float* eps_dev, float* z_out, int rows, hipStream_t s) {
    if (m->use_chain) return chain_vae_encode(m, eps_dev, z_out, rows, s);
    TRY(vae_route_check(m));
    return vae_encode_layers(m, nullptr, eps_dev, z_out, false, rows, 0, s);
}
int vae_dec_hidden(aae_model* m, int rows, hipStream_t s) {
    if (m->use_chain) return chain_vae_dec_hidden(m, rows, s);
    TRY(vae_route_check(m));
    return vae_dec_hidden_layers(m, rows, s);
}
// the cut step's first half: down to dL/d(decoder input), fc3's update (part_slabs: the fused output layer's partial slabs for
// the chain program to sum, NULL behind the three GEMMs)
int vae_backward_dec(aae_model* m, const float* part_slabs, size_t slab_stride, float* dzc_out, hipStream_t s) {
    if (!m->use_chain) { TRY(vae_route_check(m)); return vae_backward_dec_layers(m, dzc_out, s); }
    TRY(chain_vae_backward_dec(m, part_slabs, slab_stride, dzc_out, s));
    DwBuilder dw;
    dw.add(m, m->gb0.p, m->ldh, m->zc.p, m->ldc, m->rows, P_V1, O_DEC);
    return dw.launch(s);
}
// ... its second half, from the caller's dL/dz
int vae_backward_enc(aae_model* m, const float* dz_dev, int ld_dz, hipStream_t s) {
    if (!m->use_chain) { TRY(vae_route_check(m)); return vae_backward_enc_layers(m, dz_dev, ld_dz, s); }
    TRY(chain_vae_backward_enc(m, dz_dev, ld_dz, s));
    DwBuilder dw;
    dw.add(m, m->gmulv.p, (int)m->gmulv.ld, m->eh1.p, m->ldh, m->rows, P_W3, O_ENC);
    TRY(dw.add_first_layer(m, m->gb3.p, O_ENC, s)); m->w1_merged = true;
    TRY(dw.launch(s));
    return encoder_first_layer_update(m, m->gb3.p, O_ENC, s, m->w1_merged);
}
// the whole backward below the output layer (aae_vae_step)
int vae_backward(aae_model* m, const float* part_slabs, size_t slab_stride, hipStream_t s) {
    if (!m->use_chain) {
        TRY(vae_route_check(m));
        TRY(vae_backward_dec_layers(m, nullptr, s));
        return vae_backward_enc_layers(m, m->gzc.p, m->ldc, s);
    }
    TRY(chain_vae_backward(m, part_slabs, slab_stride, s));
    DwBuilder dw;
    dw.add(m, m->gb0.p, m->ldh, m->zc.p, m->ldc, m->rows, P_V1, O_DEC);
    dw.add(m, m->gmulv.p, (int)m->gmulv.ld, m->eh1.p, m->ldh, m->rows, P_W3, O_ENC);
    TRY(dw.add_first_layer(m, m->gb3.p, O_ENC, s)); m->w1_merged = true;
    TRY(dw.launch(s));
    return encoder_first_layer_update(m, m->gb3.p, O_ENC, s, m->w1_merged);
}

// ---- the decoder's hidden layers, backward (VAE cut / VAE / chain program / per-layer GEMMs)
int decoder_hidden_backward(aae_model* m, const DecodeMode& mode, const float* chain_part, size_t chain_stride, const DropSpec& d1, float* dzc_out, hipStream_t s) {
    const int B = m->rows, h = m->h, cp = m->cp;
    // cut at the condition boundary: stop at dL/d(decoder input); fc3's weight gradient + optimiser here, the rest
    // of the backward pass comes with the caller's dL/dz (aae_vae_encoder_backward)
    if (mode.vae && m->vae_cut) return vae_backward_dec(m, chain_part, chain_stride, dzc_out, s);
    if (mode.vae) return vae_backward(m, chain_part, chain_stride, s);
    if (m->use_chain) {
        // decoder hidden backward (+ the encoder backward when called from aae_step) in one program,
        // then every small weight gradient + optimiser update in one grouped launch
        const bool enc_too = mode.enc_too;
        TRY(chain_ae_backward(m, true, enc_too, chain_part, chain_stride, nullptr, 0, dzc_out, O_ENC, s, 16, enc_too));
        DwBuilder dw;
        dw_add_decoder(dw, m);
        if (enc_too) {
            TRY(dw_add_encoder(dw, m, s));
            m->enc_bwd_done = true;
        }
        return dw.launch(s);
    }
    // lin2
    EpiActBwd b1; b1.out = m->gb1.p; b1.ld = m->ldh; b1.y = m->dh1.p; b1.ldy = m->ldh; b1.act = m->cfg.activation;
    b1.d = d1; b1.seed = m->cfg.seed; b1.step_ctr = m->step_ctr;
    TRY(linear_dx(m->gb0.p, m->ldh, B, m->P[P_V2], h, b1, s, gmode(m)));
    TRY(linear_dw(m, m->gb0.p, m->ldh, B, m->dh1.p, m->ldh, P_V2, O_DEC, s));
    // lin1
    EpiStore ez; ez.out = m->gzc.p; ez.ld = m->ldc;
    TRY(linear_dx(m->gb1.p, m->ldh, B, m->P[P_V1], cp, ez, s, gmode(m)));
    TRY(linear_dw(m, m->gb1.p, m->ldh, B, m->zc.p, m->ldc, P_V1, O_DEC, s));
    if (dzc_out) {
        hipLaunchKernelGGL(copy2d_kernel, dim3(grid1d((size_t)B * cp)), dim3(256), 0, s, m->gzc.p, m->ldc, dzc_out, cp,
                           B, cp, 1.0f);
        LAUNCHCHK("copy dzc");
    }
    return AAE_OK;
}

// ---- the decode-backward phase: decoder hidden layers forward (unless they ran, or ACT_DH2 is the input), the output layer,
// the decoder's hidden layers backward.  mode: what the entry point that makes the call wants beyond the plain phase
int decode_backward(aae_model* m, const float* zc_dev, int64_t zc_ld, const aae_rng_inject* inj, float* dzc_out,
                    const DecodeMode& mode, hipStream_t s) {
    if (m->phase != 1) return fail(AAE_ESTATE, "aae_ae_decode_backward without aae_ae_encode");
    remember_inject(m, inj, false);
    const int B = m->rows, N = m->N, h = m->h;
    if (zc_dev) TRY(stage_zc(m, zc_dev, zc_ld, B, s));
    const uint8_t* mk2 = m->inj.masks_dev[2];
    const uint8_t* mk3 = m->inj.masks_dev[3];
    if (mode.only_output_layer || mode.vae) { /* ACT_DH2 is the input / the VAE's entry points ran its one hidden layer */ }
    else if (m->use_chain) { if (!m->dec_hidden_done) TRY(chain_dec_hidden(m, true, B, s)); }
    else TRY(decoder_hidden_forward(m, true, mk2, mk3, B, s));
    TRY(join_output_layer(m, s));       // a deferred launch of the step before that was left running at this step's opening (late join)
    const float gscale = m->grad_scale / ((float)B * (float)N);
    DropSpec d1 = make_drop(m, 0, true, mk2, nullptr, B, h, 2);
    DropSpec d2 = make_drop(m, 1, true, mk3, nullptr, B, h, 3);
    const float* chain_part = nullptr; size_t chain_stride = 0;
    const OutForm form = output_form(m);
    if (form == OutForm::Three) TRY(output_layer_unfused(m, mode, B, gscale, d2, s));
    else TRY(output_layer_fused(m, form, mode, B, gscale, d2, &chain_part, &chain_stride, s));
    if (!mode.only_output_layer) TRY(decoder_hidden_backward(m, mode, chain_part, chain_stride, d1, dzc_out, s));
    m->phase = 2;
    return AAE_OK;
}

}  // namespace

extern "C" {

int aae_ae_decode_backward(aae_handle m, const float* zc_dev, int64_t zc_ld, const aae_rng_inject* inj,
                           float* dzc_out, void* stream) {
    if (!m) return fail(AAE_EINVAL, "handle is NULL");
    return decode_backward(m, zc_dev, zc_ld, inj, dzc_out, DecodeMode{}, S(stream));
}

}  // extern "C"
