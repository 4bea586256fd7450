// libaaerec_hip.so - C ABI (include/aaerec_hip.h) and step orchestration.
//
// One `aae_model` = the three nets + four optimisers that AdversarialAutoEncoder.fit builds
// (reference aaerec/aae.py:782-804), laid out in one caller-owned HBM arena:
//
//   parameters      item-major for the two vocabulary-sized layers (ENC_W1T [N][h], DEC_V3
//                   [N][h+1]) so that a gathered / streamed row is one contiguous 800-byte line;
//                   every other Linear "augmented" [out][in+1] (bias = last column) so that the
//                   forward GEMM adds the bias and the weight-gradient GEMM yields the bias
//                   gradient for free (activations carry a constant-1 column).
//   optimiser state exp_avg / exp_avg_sq with the layout of their parameter, two independent
//                   states for the encoder (enc_optim, gen_optim; aae.py:800,803).
//   activations     fp32 [rows][ld], ld = round4(width+1).
//
// The step is a fixed sequence of kernel launches on one stream (no host sync, no allocation),
// so a caller may capture it into a hipGraph.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/aaerec_hip.h"
#include "gemm_f32.h"
#include "kernels.h"
#include "dec_fused.h"
#include "dec_fused_bf16.h"
#include "dec_crit_x3.h"
#include "rank_x3.h"
#include "rank_long.h"
#include "rank_full.h"
#include "loss_eval.h"
#include "cooc.h"
#include "spgemm.h"
#include "sptrans.h"
#include "mutinfo.h"
#include "popular.h"
#include "randrank.h"
#include "rank_metrics.h"
#include "lowrank.h"
#include "irgan.h"
#include "chain.h"
#include "chain4.h"
#include "chain16x3.h"
#include "vae_layers.h"
#include "cond_embed.h"
#include "cond_bag.h"
#include "cond_csr.h"
#include "cond_gather.h"
#include "w1_update.h"
#include "dae_corrupt.h"

using namespace aae;

#include "kernel_pick.h"

#include <map>
static std::map<std::string, std::string> g_options;      // aae_set_option: name -> value (wins over the environment)
const char* option_value(const char* name) {
    auto it = g_options.find(name);
    if (it != g_options.end()) return it->second.c_str();
    return getenv((std::string("AAE_") + name).c_str());
}

#include "abi_model.h"
#include "abi_layers.h"
#include "abi_chains.h"
#include "abi_rank.h"

// ------------------------------------------------------------------------------------------
extern "C" {

int aae_abi_version(void) { return AAE_ABI_VERSION; }

int aae_set_option(const char* name, const char* value) {
    if (!name || !*name) return fail(AAE_EINVAL, "option name is empty");
    static const char* known[] = {"NO_CHAIN", "CHAIN16", "SPLIT_ANY", "BLOCKED_ANY", "EARLY_ANY", "NO_LATE_JOIN", "NO_ITEM_COUNT", "NO_ITEM_LISTS", "NO_INLINE_PREFETCH", "INLINE_PF_DISC8", "W1_SERIAL",
                                  "NO_RANK_FUSED", "CHAIN_KSLICES", "X16_ROWS", "DW_KSPLIT_ROWS", "DEC_TS", "CHAIN_TS", "DW_TS", "DEC_SKIP", "CHAIN_SKIP", "RANK_SKIP",
                                  "RANK_COLLECT_CAP"};
    bool ok = false;
    for (const char* k : known) ok = ok || strcmp(k, name) == 0;
    if (!ok) return fail(AAE_EINVAL, "unknown option (aae_options, csrc/abi_model.h, lists them)");
    if (value && strcmp(name, "RANK_COLLECT_CAP") == 0) {      // (a whole number of list entries the LDS sort can hold)
        char* end = nullptr;
        const long v = strtol(value, &end, 10);
        if (end == value || *end || v < 1 || v > kLongCap) return fail(AAE_EINVAL, "RANK_COLLECT_CAP must be a whole number in [1, 4096]");
    }
    if (value) g_options[name] = value; else g_options.erase(name);
    return AAE_OK;
}
const char* aae_last_error(void) { return g_err.c_str(); }

int aae_arena_bytes(const aae_config* cfg, size_t* bytes_out) {
    TRY(validate(cfg));
    if (!bytes_out) return fail(AAE_EINVAL, "bytes_out is NULL");
    aae_model tmp; memset((void*)&tmp, 0, sizeof(tmp)); tmp.cfg = *cfg;
    read_options(tmp.opt);
    *bytes_out = layout(&tmp, nullptr, true);
    return AAE_OK;
}

int aae_create(const aae_config* cfg, void* arena_dev, size_t arena_bytes, void* stream, aae_handle* out) {
    TRY(validate(cfg));
    if (!arena_dev || !out) return fail(AAE_EINVAL, "arena/out is NULL");
    if (reinterpret_cast<uintptr_t>(arena_dev) & 255) return fail(AAE_EINVAL, "arena must be 256-byte aligned");
    aae_model* m = new aae_model();
    memset((void*)m, 0, sizeof(*m));
    m->cfg = *cfg;
    read_options(m->opt);                // every switch of the library, once per handle (abi_model.h aae_options)
    size_t need = layout(m, static_cast<char*>(arena_dev), false);
    if (need > arena_bytes) { delete m; return fail(AAE_ENOMEM, "arena smaller than aae_arena_bytes()"); }
    m->base = static_cast<char*>(arena_dev); m->bytes = need;
    m->alpha_mode = cfg->activation == AAE_ACT_SELU;
    m->vae = cfg->model_kind == 3; m->vae_cut = false;
    m->bf16 = cfg->dtype == 1;
    m->split_any = m->opt.split_any;
    m->x3_gemm = !m->bf16;
    m->noise_next = nullptr; m->noise_ld = 0; m->dense_step = false; m->noise_gen_next = false; m->noise_gen_scale = 0.f;
    m->ae_only = cfg->model_kind == 1 || m->vae;
    m->lazy = true;    // deferred Adam on W1T in both gradient modes (export mode exchanges packed rows)
    // the dynamic-LDS limit of a kernel family (kernel_pick.h each_*): a failure clears the capability flag it belongs to.
    // Every output-layer family gets the chip's whole LDS (a launch asks for its family's own *_lds_bytes)
    auto limit = [](bool& ok, size_t bytes) { return [&ok, bytes](auto kernel) { ok = ok && raise_lds_limit(kernel, bytes); }; };
    const int maxlds = 160 * 1024;
    {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) {
            delete m; return fail(AAE_EHIP, "no HIP device");
        }
        m->n_cu = std::min(cus, 304);
        const int nb = (m->h + 1 + 15) / 16;
        m->fused_nb = nb <= 4 ? 4 : nb <= 7 ? 7 : nb <= 13 ? 13 : 0;
        m->fused_ok = m->fused_nb != 0 && fused_width_ok(m->h, m->ldh);       // (the arena's slab area is sized by the same test)
        // (a decoder input [z | condition | 1] of up to 2 x 208 columns: two k-parts on the 4-row kernel; a VAE handle's: up to
        //  kVaeInParts parts on the 16-row kernel, abi_chains.h)
        m->use_chain = (m->h + 1 <= 208) && (m->c + 1 <= 208) && (m->cp + 1 <= (m->vae ? kVaeDecInMax : 2 * 208)) &&
                       !m->opt.no_chain;      // (the code itself has to fit a slot: only the condition block may exceed it)
        if (m->vae && !vae_fits_chain(m->h, m->c)) m->use_chain = false;      // (cfg.vae_wide: [mu | logvar] has to fit a slot as well)
        const size_t chain_lds = kCSlots * kCR * kCL * sizeof(float);
        if (m->use_chain) each_chain(false, limit(m->use_chain, chain_lds));
        // (the r6 activation classes live in chain_kernel<.., true> alone: device_common.h act_fwd)
        m->act_nm = cfg->activation > AAE_ACT_LEAKYRELU;
        if (m->use_chain && m->act_nm) each_chain(true, limit(m->use_chain, chain_lds));
        m->use_chain4 = m->use_chain && !m->act_nm && !m->opt.chain16;
        if (m->use_chain4) each_chain4(limit(m->use_chain4, chain_lds));
        if (m->use_chain && m->cp + 1 > 208 && !m->use_chain4 && !m->vae) m->use_chain = false;      // (the AAE's two k-parts: chain4.h alone)
        // a cfg.vae_wide handle off the chain programs (its sizes, or NO_CHAIN): the per-layer route.  What launch_gather asks of
        // enc_gather_kernel_t<16> for a row's image (gather_lds_bytes; + the kernel's 64 bytes of static LDS) passes the default
        // 64 KB at the widest hidden layer: the limit is raised to that request here, the only place that does so for this kernel
        // (the four-wave form of batches from 512 rows on asks for a quarter and stays below)
        m->vae_layers = m->vae && cfg->vae_wide == 1 && !m->use_chain;
        if (m->vae_layers && gather_lds_bytes(m->h) + 64 > 64 * 1024) {
            bool ok = true;
            limit(ok, gather_lds_bytes(m->h))(enc_gather_kernel_t<16>);
            (void)hipGetLastError();
            if (!ok) { delete m; return fail(AAE_EHIP, "the first layer's gather cannot take the LDS of this n_hidden"); }
        }
        m->x16_rows = m->opt.x16_rows;
        m->dw_ksplit_rows = 256;                       // (the handle is zero-filled after construction: no default member values)
        if (m->opt.dw_ksplit_rows >= 0) m->dw_ksplit_rows = m->opt.dw_ksplit_rows;
        if (!m->opt.no_item_count) {
            void* hp = nullptr; void* dp = nullptr;
            if (hipHostMalloc(&hp, 64, hipHostMallocMapped) == hipSuccess && hipHostGetDevicePointer(&dp, hp, 0) == hipSuccess) {
                m->cnt_host = static_cast<int*>(hp); m->cnt_host_dev = static_cast<int*>(dp); *m->cnt_host = 0;
            } else { if (hp) (void)hipHostFree(hp); (void)hipGetLastError(); }
        }
        m->x16_ok = m->use_chain4 && m->FXi[P_W2] != nullptr;
        if (m->x16_ok) each_chain16x3(limit(m->x16_ok, kX16Lds));
        m->force_unfused = cfg->unfused_decoder == 1;   // debugging / A-B switch: unfused_decoder = 1 keeps the 3-kernel path
        if (m->fused_ok) {
            each_dec_fused(limit(m->fused_ok, maxlds));
            if (m->bf16) each_dec_fused_bf16(limit(m->fused_ok, maxlds));
            if (!raise_lds_limit(tile_bucket_kernel, maxlds - 2048)) m->fused_ok = false;
            m->bucket_wide_ok = raise_lds_limit(tile_bucket_wide_kernel, maxlds - 16384);
            {   //  the wide bucket builder keeps other workgroups off its CU by its register count (buckets.h: a clobber of
                // v127) on top of its LDS claim: say so once if a compiler stops honouring the clobber - results do not depend on it
                hipFuncAttributes fa;
                static bool told = false;
                if (m->bucket_wide_ok && !told && hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(tile_bucket_wide_kernel)) == hipSuccess && fa.numRegs < 121) {
                    told = true;
                    fprintf(stderr, "aaerec: tile_bucket_wide_kernel allocates %d vector registers, not the 128 it claims to keep its CU to itself (buckets.h)\n", fa.numRegs);
                }
                (void)hipGetLastError();
            }
        }
    }
    m->late_enabled = !m->opt.no_late_join;
    m->early_enabled = true;
    m->early_any = m->opt.early_any;        // (tests: the early prefetch at every batch size)
    m->rank_ok = m->fused_ok && m->use_chain4 && !m->vae && !m->opt.no_rank_fused;      // (the rank kernels' limit: what they launch with)
    // (a VAE handle ranks through the aae_vae_* calls alone: its hidden half is another program, on the 4-row kernel's VAE member)
    m->vae_rank_ok = m->vae && m->fused_ok && m->use_chain4 && !m->opt.no_rank_fused;
    if (m->vae_rank_ok) each_chain4_vae(limit(m->vae_rank_ok, kCSlots * kCR * kCL * sizeof(float)));
    bool& rank_ok = m->vae ? m->vae_rank_ok : m->rank_ok;
    if (rank_ok) each_rank([&](const RankPick& r) { rank_ok = rank_ok && raise_lds_limit(r.kernel, r.lds); });
    m->w1_big_lds = raise_lds_limit(w1_item_update_kernel, sizeof(int) * w1_items_lds_words(16384));
    (void)hipGetLastError();
    m->grad_scale = 1.f;
    m->rng_row0 = 0; m->rng_global = 0;
    m->Gt = m->G.p;
    m->split_ok = false; m->opt_pending = false; m->side = nullptr; m->ev_crit = m->ev_opt = nullptr;
    // workgroups of the deferred optimiser launch.  r2: half the CUs (it had 50 us of slack then).  Since the critical launch
    // runs on the bf16 matrix cores (r3, 116 -> 84 us) the NEXT step waits for this launch; measured at C3, batch 100
    // (r2-r3 sweep of the launch's width, ms/step), with the fp32 deferred kernel: 112 0.306 | 128 0.291 | 144 0.274 | 160 0.274 | 176 0.284
    // | 192 0.285 | 224 0.312; with the bf16-emulated one (dec_opt_x3_kernel: 160 -> 138 us on 128 workgroups): 112 0.279 |
    // 128 0.273 | 144 0.276 | 160 0.278 | 176 0.286.  Half the CUs again (set below once split_ok is known):
    // beyond that the chain / weight-gradient kernels it runs beside lose more than the launch gains.
    m->split_wgs = std::max(1, (m->n_cu * 5) / 8);
    m->pf_armed = m->pf_built = m->pf_pending = false; m->pf_step = -1; m->hstep = 0; m->flushed_hstep = -1; m->ev_head = m->ev_pf = nullptr;
    bool side_ok = false;
    if (cfg->grad_mode == AAE_GRAD_FUSED) {
        // the handle's side stream (lowest priority) for work off the step's critical path: the deferred optimiser
        // launch of the output layer and the next batch's deferred-Adam catch-up.  The events order work of this device
        // only: no system-scope release (an L2 write-back) at the record
        int lo = 0, hi = 0;
        const unsigned evflags = hipEventDisableTiming | hipEventDisableSystemFence;
        side_ok = hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess &&
                  hipStreamCreateWithPriority(&m->side, hipStreamNonBlocking, lo) == hipSuccess &&
                  hipEventCreateWithFlags(&m->ev_crit, evflags) == hipSuccess &&
                  hipEventCreateWithFlags(&m->ev_opt, evflags) == hipSuccess &&
                  hipEventCreateWithFlags(&m->ev_head, evflags) == hipSuccess &&
                  hipEventCreateWithFlags(&m->ev_pf, evflags) == hipSuccess &&
                  hipEventCreateWithFlags(&m->ev_bk, evflags) == hipSuccess &&
                  hipEventCreateWithFlags(&m->ev_end, evflags) == hipSuccess;
        if (!side_ok) {
            if (m->side) (void)hipStreamDestroy(m->side);
            m->side = nullptr;
        }
        (void)hipGetLastError();
    }
    // The split forms of the output layer exist - ONE capability: the side stream and its events, the single launch (the bucket
    // build and the slab area are its), the stored dL/dlogits tiles of a row block behind one descriptor, and the LDS limit of
    // every dec_crit_x3.h family this handle's dtype launches: critical, deferred, blocked-deferred.
    // (a bf16 handle runs the same kernels with every operand rounded to bf16 - DecFusedArgs::one_term - and the critical and
    //  deferred launch on their one-term instantiations, ONE matrix instruction per product.  Both launches got faster with them -
    //  critical 35 -> 27 us, deferred 85 -> 74 us at C2 - and for most of r4 the STEP got slower, 0.173 -> 0.186 ms
    //  (r4's profile of C2 in bf16 under profiles/): the one-term deferred kernel needs 78 VGPRs instead of 126, so six of its waves fit a
    //  SIMD, its 1024-thread workgroup no longer fills its CU, and the dispatcher deals the step's own weight-gradient / gather
    //  workgroups onto the CUs where it streams 24 B per parameter (the weight-gradient launch beside it: 32 us instead of 11).
    //  Its launch now claims 150 KB of LDS (abi_output_layer.h), which no other workgroup of the step fits beside: 0.1648 ms at
    //  the old width, 0.162-0.164 on 48-64 workgroups (r4 sweep; a claim of 120 KB leaves the 24 KB
    //  weight-gradient workgroups in: 0.1865).)
    // (dec_opt_x3_kernel's three-term instantiations take 123 648 bytes - the 58 112 of the tile and 64 KB for the third term of
    //  dh2's fragments)
    if (side_ok && m->fused_ok &&
        (size_t)((m->N + kTI - 1) / kTI) * kTI * (size_t)std::min(m->R, 16 * kMB) * sizeof(float) < (size_t)0x7FFFFFF0u) {
        m->split_ok = true;
        each_dec_crit_x3(m->bf16, limit(m->split_ok, maxlds));
        each_dec_opt_x3(m->bf16, limit(m->split_ok, maxlds));
        each_dec_opt_blocks_x3(limit(m->split_ok, maxlds));
        (void)hipGetLastError();
        if (m->split_ok) {
            // Workgroups of the deferred launch (batches of one fused launch).  It has to end before the step does (the next
            // step opens behind it), and every CU it holds is one the step's own launches share with it: wide enough to take
            // ~80 us - every shape's step has that much work left behind the critical launch - and never more than 9/16 of
            // the chip.  A tile of 32 items costs a workgroup 3.3 us + 13 ns per hidden unit (measured: 5.9 us at 200, 4.6 us
            // at 100).  tools/debug/sweep_split_wgs*.sh, r3: C3 (3125 tiles, 200) 128 -> 0.2652-0.2733 ms/step, 144 ->
            // 0.2651-0.2655, 160 -> 0.2683, 176 -> 0.282; C2 (1469 tiles, 100) 64 -> 0.1806, 80 -> 0.1710, 96 -> 0.1721,
            // 128 -> 0.177, 160 -> 0.185.
            // Since the launch requests a tile's streams a tile ahead and deals the requests over the matrix phase
            // (dec_crit_x3.h) a tile costs 2.2 us + 9.6 ns per hidden unit on 112-120 workgroups (tools/dec_opt_width_table.py:
            // 4.11 us at 200, 3.15 at 100, one-term 3.1 at 100; 3.34 / 2.83 / 2.60 on 32 workgroups) - 0.69 of the above, and
            // the targets went down with it (57 / 127 us for 82 / 165), so that a shape nobody swept again keeps its width.
            const int ntiles = (m->N + 31) / 32;
            const double t_tile = (2.2 + 0.0096 * m->h) * (m->bf16 ? 0.98 : 1.0);
            int w = (int)(ntiles * t_tile / (m->bf16 ? 127.0 : 57.0) / 8.0 + 0.5) * 8;      // (C3's shape in bf16: 0.2230 / 0.2264 / 0.2317 / 0.2374 ms on 96 / 112 / 128 / 144)
            // (C2 in bf16, formula: 32, with the tile-ahead launch, tools/split_width_sweep.py, two passes: 0.1532-0.1534 | 0.1542-
            //  0.1549 | 0.1553-0.1556 | 0.1554-0.1556 | 0.1556-0.1560 | 0.1563-0.1565 | 0.157 | 0.157 | 0.158 ms/step on 40 | 48 | 56 |
            //  64 | 72 | 80 | 88 | 96 | 104-128: the floor of the one-term launch 48 -> 40)
            w = std::max(w, std::min(ntiles, m->bf16 ? 40 : 64));
            // r4, late join (abi_model.h: the launch may run on into the next step's forward pass, so it need not end with the
            // step): half the chip at most - C3 0.2493 (early join, 144) -> 0.2430 ms/step on 128; 0.2515 / 0.2483 / 0.2497 /
            // 0.2492 on 112 / 120 / 136 / 144 (sharp: 124 -> 0.2459, 132 -> 0.2503); the early join on 128: 0.2608.  C2 (formula:
            // 80) is flat from 64 to 96 either way (tools/debug/late_join_sweep*.sh).
            // r5: the deferred launch no longer requests the 416 float4 slots beyond a tile's span (it read 1.25x the layer): 139.7 ->
            // 130.9 us on 128 workgroups, and the optimum moved down with it - same box, C3: 0.2469 / 0.2359 / 0.2368 / 0.2386 / 0.2378 /
            // 0.2412 ms/step on 104 / 112 / 120 / 124 / 128 / 136 (tools/debug/sweep_split_wgs.sh): 15/32 of the chip
            // The tile-ahead launch (110.9 us instead of 126.7 on 120 workgroups, the launch alone): the optimum moved down again -
            // same box, C3, two passes: 0.2652 / 0.2523 / 0.2423 / 0.2339 / 0.2259 / 0.2255 / 0.2266 / 0.2284 / 0.2331 and 0.2646 /
            // 0.2520 / 0.2423 / 0.2341 / 0.2255 / 0.2262 / 0.2270 / 0.2281 / 0.2330 ms/step on 72 / 80 / 88 / 96 / 104 / 112 / 120 /
            // 128 / 136 (the launch before it: 0.2434 / 0.2327 / 0.2294 / 0.2313 and 0.2438 / 0.2326 / 0.2289 / 0.2314 on 104 / 112 /
            // 120 / 128).  104 and 112 tie and 96 is over the edge: 112, 7/16 of the chip
            // With the next batch's item list and catch-up inside the step's own chain launches (abi_chains.h: inline_prefetch_applies;
            // nothing of them is left on the side stream in front of this launch or beside the critical one) the optimum moved down
            // once more - same box, C3, two passes: 0.2420 / 0.2324 / 0.2237 / 0.2206 / 0.2175 / 0.2183 / 0.2188 / 0.2227 / 0.2258 and
            // 0.2420 / 0.2323 / 0.2236 / 0.2203 / 0.2176 / 0.2184 / 0.2191 / 0.2221 / 0.2258 ms/step on 80 / 88 / 96 / 100 / 104 /
            // 108 / 112 / 120 / 128 (the side-stream route on the same build: 0.2214-0.2217 / 0.2233-0.2236 on 112 / 120; the build
            // before it: 0.2345 / 0.2273 / 0.2214 / 0.2232 on 96 / 104 / 112 / 120): 104, 13/32 of the chip, for the handles that
            // take that route; the others keep 112.  C2 in bf16 keeps its 40 (0.1629 / 0.1470 / 0.1488 / 0.1498 on 32 / 40 / 48 / 56).
            // (profiles/inline_prefetch_width_sweep.txt)
            const int cap = !m->late_enabled ? m->n_cu * 9 / 16 : inline_prefetch_handle(m) ? m->n_cu * 13 / 32 : m->n_cu * 7 / 16;
            m->split_wgs = std::max(1, std::min(w, cap));
        }
    }
    hipStream_t s = S(stream);
    hipError_t e = hipMemsetAsync(arena_dev, 0, need, s);
    if (e != hipSuccess) { delete m; return fail(AAE_EHIP, std::string("hipMemsetAsync: ") + hipGetErrorString(e)); }
    // constant-1 columns of the activation buffers that feed augmented weights
    struct { Ten* t; int col; } ones[] = {{&m->eh1, m->h}, {&m->eh2, m->h}, {&m->zc, m->cp}, {&m->dh1, m->h},
                                           {&m->dh2, m->h}, {&m->zin, m->c}, {&m->xh1, m->h}, {&m->xh2, m->h}};
    for (auto& o : ones)
        hipLaunchKernelGGL(fill_col_kernel, dim3(((int)o.t->rows + 255) / 256), dim3(256), 0, s, o.t->p, (int)o.t->ld,
                           (int)o.t->rows, o.col, 1.0f);
    OptScalars hs[4]; memset(hs, 0, sizeof(hs));
    for (int i = 0; i < 4; ++i) {
        hs[i].t = 0; hs[i].is_sgd = cfg->optimizer == AAE_OPT_SGD;
        hs[i].lr = (i == O_ENC || i == O_DEC) ? (double)cfg->gen_lr : (double)cfg->reg_lr;
        hs[i].neg_step_size = 0.f; hs[i].bc2_sqrt = 1.f; hs[i].inv_bc2_sqrt = 1.f;
    }
    e = hipMemcpyAsync(m->sc, hs, sizeof(hs), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { delete m; return fail(AAE_EHIP, std::string("init: ") + hipGetErrorString(e)); }
    *out = m;
    return AAE_OK;
}

#ifdef W1_TS
int aae_debug_w1_ts(unsigned long long* out, int n) {      // (debug builds only)
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(aae::w1_ts), sizeof(unsigned long long) * (size_t)n);
}
#endif
int aae_destroy(aae_handle h) {
    if (!h) return AAE_OK;
    if (h->side) {
        (void)hipStreamSynchronize(h->side);     // the arena is the caller's: nothing of ours may still write it
        (void)hipStreamDestroy(h->side);
    }
    if (h->dp_scratch) (void)hipFree(h->dp_scratch);
    if (h->cnt_host) (void)hipHostFree(h->cnt_host);
    for (hipEvent_t e : {h->ev_crit, h->ev_opt, h->ev_head, h->ev_pf, h->ev_bk, h->ev_end}) if (e) (void)hipEventDestroy(e);
    if (h->prof_ev) {
        for (int k = 0; k < AAE_K_N; ++k)
            for (auto& pr : h->prof_ev[k]) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
        delete[] h->prof_ev;
    }
    delete h;
    return AAE_OK;
}


int aae_profile_enable(aae_handle h, int on) {
    if (!h) return fail(AAE_EINVAL, "handle is NULL");
    if (on && !h->prof_ev) h->prof_ev = new std::vector<std::pair<hipEvent_t, hipEvent_t>>[AAE_K_N];
    h->prof_on = on != 0;
    h->prof_mask = on == 1 ? ~0u : ((unsigned)on >> 1);     // 1 = every kernel id; else bit (k + 1) selects id k
    return AAE_OK;
}

int aae_profile_read(aae_handle h, int kernel_id, double* total_ms, int64_t* launches) {
    if (!h || !total_ms || !launches) return fail(AAE_EINVAL, "NULL argument");
    if (kernel_id < 0 || kernel_id >= AAE_K_N) return fail(AAE_EINVAL, "bad kernel id");
    *total_ms = 0.0; *launches = 0;
    if (!h->prof_ev) return AAE_OK;
    auto& v = h->prof_ev[kernel_id];
    for (size_t i = 0; i < h->prof_used[kernel_id]; ++i) {
        HIPCHK(hipEventSynchronize(v[i].second));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, v[i].first, v[i].second));
        *total_ms += ms; *launches += 1;
    }
    h->prof_used[kernel_id] = 0;
    return AAE_OK;
}

int aae_prefetch_batch(aae_handle h, const aae_batch* next) {
    if (!h || !next) return fail(AAE_EINVAL, "NULL argument");
    if (!next->indptr_dev || !next->indices_dev || !next->values_dev) return fail(AAE_EINVAL, "batch pointers are NULL");
    if (next->n_rows < 1 || next->n_rows > h->R) return fail(AAE_EINVAL, "batch n_rows outside [1, max_batch]");
    if (next->nnz_bound > h->cfg.max_nnz) return fail(AAE_EINVAL, "batch nnz_bound > max_nnz");
    if (next->generation == 0) { h->pf_armed = false; return AAE_OK; }      // (no content id: no step could ever match it)
    h->pf_batch = *next;
    h->pf_armed = true;
    return AAE_OK;
}

int aae_set_input_noise(aae_handle h, const float* noise_dev, int64_t noise_ld) {
    if (!h) return fail(AAE_EINVAL, "handle is NULL");
    if (!h->Xn.p) return fail(AAE_ESTATE, "aae_set_input_noise: the model was not created with cfg.dense_noise = 1");
    if (noise_dev && noise_ld < h->N) return fail(AAE_EINVAL, "noise_ld < n_items");
    h->noise_next = noise_dev; h->noise_ld = noise_ld;
    h->noise_gen_next = false;                 // (a pending aae_set_input_noise_gen is replaced: the later call wins)
    return AAE_OK;
}

// ... the deferred optimiser launch alone (activation views: the next batch's prefetch - aae_prefetch_batch - touches
// enc.lin1 and its bookkeeping only, and keeps running beside the step)
int aae_join_output_layer(aae_handle h, void* stream) {
    if (!h) return fail(AAE_EINVAL, "handle is NULL");
    // (only the optimiser launch is settled here.  A prefetch enqueued BEHIND it - an item slice's, pf_after_opt - is not
    //  covered by ev_opt and stays pending for the next step's join_deferred; one enqueued in front of it - aae_step's -
    //  is covered by the later record of the in-order side stream)
    if (h->opt_pending) {
        HIPCHK(hipStreamWaitEvent(S(stream), h->ev_opt, 0));
        h->opt_pending = false;
        if (!h->pf_after_opt) h->pf_pending = false;
    }
    return AAE_OK;
}

int aae_join(aae_handle h, void* stream) {
    if (!h) return fail(AAE_EINVAL, "handle is NULL");
    return join_deferred(h, S(stream));
}

int aae_set_split(aae_handle h, int32_t workgroups) {
    if (!h) return fail(AAE_EINVAL, "handle is NULL");
    if (workgroups < 0) return fail(AAE_EINVAL, "workgroups must be >= 0");
    if (h->opt_pending) return fail(AAE_ESTATE, "aae_set_split with a deferred launch pending: call aae_join / aae_sync first");
    h->split_wgs = workgroups;
    return AAE_OK;
}

int aae_set_grad_scale(aae_handle h, float scale) {
    if (!h) return fail(AAE_EINVAL, "handle is NULL");
    h->grad_scale = scale; return AAE_OK;
}

// learning rates are float32 in aae_config; callers that need the exact Python double can set it here
int aae_set_rng_rows(aae_handle h, int64_t row_offset, int64_t global_rows) {
    if (!h) return fail(AAE_EINVAL, "handle is NULL");
    if (row_offset < 0 || global_rows < 0 || row_offset > (1 << 30) || global_rows > (1 << 30))
        return fail(AAE_EINVAL, "aae_set_rng_rows: bad offset / global_rows");
    h->rng_row0 = (int)row_offset; h->rng_global = (int)global_rows;
    return AAE_OK;
}

int aae_params_changed(aae_handle h) {
    if (!h) return fail(AAE_EINVAL, "handle is NULL");
    for (int i = 0; i < NP; ++i) h->pt_ok[i] = false;
    return AAE_OK;
}

int aae_set_lr(aae_handle h, double gen_lr, double reg_lr) {
    if (!h) return fail(AAE_EINVAL, "handle is NULL");
    TRY(join_host(h));
    OptScalars hs[4];
    HIPCHK(hipMemcpy(hs, h->sc, sizeof(hs), hipMemcpyDeviceToHost));
    hs[O_ENC].lr = gen_lr; hs[O_DEC].lr = gen_lr; hs[O_GEN].lr = reg_lr; hs[O_DISC].lr = reg_lr;
    HIPCHK(hipMemcpy(h->sc, hs, sizeof(hs), hipMemcpyHostToDevice));
    h->spec_tab_ok = false;             // (the table entry written a step early was computed with the old rates)
    return AAE_OK;
}

int aae_tensor_info(aae_handle h, int id, aae_tensor* out) {
    if (!h || !out) return fail(AAE_EINVAL, "handle/out is NULL");
    const Ten* t = nullptr;
    Ten tmp;
    auto adam = [&](int base, int lo, int hi, int set) -> const Ten* {
        int k = id - base, pid = lo + k / 2;
        if (k < 0 || pid > hi) return nullptr;
        return (k & 1) ? &h->V[set][pid] : &h->M[set][pid];
    };
    if (id >= 0 && id < AAE_T_N_PARAMS) t = &h->P[id];
    else if (id >= AAE_T_ADAM_ENC && id < AAE_T_ADAM_ENC + 8) t = adam(AAE_T_ADAM_ENC, P_W1T, P_W3, 0);
    else if (id >= AAE_T_ADAM_GEN && id < AAE_T_ADAM_GEN + 8) t = adam(AAE_T_ADAM_GEN, P_W1T, P_W3, 1);
    else if (id >= AAE_T_ADAM_DEC && id < AAE_T_ADAM_DEC + 6) t = adam(AAE_T_ADAM_DEC, P_V1, P_V3, 0);
    else if (id >= AAE_T_ADAM_DISC && id < AAE_T_ADAM_DISC + 6) t = adam(AAE_T_ADAM_DISC, P_D1, P_D3, 0);
    else if (id >= AAE_T_GRAD && id < AAE_T_GRAD + NP) { t = &h->Gr[id - AAE_T_GRAD]; if (!t->rows) t = nullptr; }
    else if (id == AAE_T_ACT_Z) t = &h->zsave;
    else if (id == AAE_T_ACT_A1) t = &h->a1;
    else if (id == AAE_T_ACT_DH2) t = &h->dh2;
    else if (id == AAE_T_ACT_DA2) t = &h->da2;
    // (ga1x: the LAST rows hold the batch; the per-layer path - NO_CHAIN, or a model too wide for the chain programs - leaves
    //  dL/d(a1) in gb1: abi_layers.h encoder_backward)
    else if (id == AAE_T_ACT_GA1) t = (h->ext_first && h->ga1x.p) ? &h->ga1x : (h->use_chain || h->vae_layers) ? &h->gb3 : &h->gb1;
    else if (id == AAE_T_ACT_DZC) { tmp = h->gzc; tmp.cols = h->cp; t = &tmp; }
    else if (id == AAE_T_ACT_LOSSES) {
        tmp.rows = 1; tmp.cols = 4; tmp.ld = 4; tmp.off = (size_t)((char*)h->losses - h->base); t = &tmp;
    }
    else if (id == AAE_T_W1_TSYNC && h->lazy) {
        tmp.rows = 1; tmp.cols = h->N; tmp.ld = h->N; tmp.off = (size_t)((char*)h->tsync - h->base); t = &tmp;
    }
    if (!t) return fail(AAE_EINVAL, "unknown tensor id");
    out->byte_offset = t->off; out->rows = t->rows; out->cols = t->cols; out->ld = t->ld;
    return AAE_OK;
}

// brings every deferred update up to date so that the arena views of ENC_W1T and its optimiser
// state hold the values an eager implementation would
int aae_sync(aae_handle h, void* stream) {
    if (!h) return fail(AAE_EINVAL, "handle is NULL");
    TRY(join_deferred(h, S(stream)));
    return lazy_flush(h, S(stream));
}


}  // extern "C"

#include "abi_condition.h"
#include "abi_state_dict.h"
#include "abi_dae.h"
#include "abi_step_open.h"
#include "abi_output_layer.h"
#include "abi_step_phases.h"
#include "abi_predict.h"
#include "abi_cooc.h"
#include "abi_spgemm.h"
#include "abi_sptrans.h"
#include "abi_mutinfo.h"
#include "abi_popular.h"
#include "abi_random.h"
#include "abi_metrics.h"
#include "abi_lowrank.h"
#include "abi_irgan.h"
#include "abi_data_parallel.h"

#include "dp_step.h"
#include "ipc_collectives.h"
