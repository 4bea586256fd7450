// Per-batch item row lists for the first encoder layer's update (w1_update.h), built ONCE per batch and off the step's
// critical path.
//
// Everything the hybrid form (w1_item_hybrid_body) does up to "which rows hold this item, in ascending order, with which
// value" depends on the batch alone - not on dL/d(a1), the weights or the optimiser - and was computed twice per step
// (enc_optim's and gen_optim's update), inside launches the whole step waits for, as a chain of dependent memory round trips:
// count -> item id -> tile range -> entries -> row scales and rows.  Here extra workgroups of the ae phase's backward chain
// launch (chain4.h; ~25 row workgroups beside > 100 idle CUs) build one fixed-size RECORD per entry of the distinct-item list:
//
//   word 0      item id
//   word 1      n, the number of batch rows that hold it
//   word 2      n > kW1HybRows: its overflow slot
//   words 4-7   n <= kW1HybRows: its rows, ascending, one byte each (a fused launch's batch has at most 112 rows)
//   words 8-23  ... and value * rscale[row] of each (the one fp32 multiply the update did itself)
//
// An item with more rows gets an OVERFLOW SLOT with its full ascending (row, scaled value) list; the slots are handed out by
// an atomic counter, so their order is arbitrary - items are independent.  The lists are derived exactly as the update derives
// them: ballot + prefix popcount over the tile bucket and the rank by row (small items), bitmap + prefix popcounts (the others).
//
// The consumers (grouped_dw_kernel's first-layer workgroups) are then two round trips deep: record, then dL/d(a1) rows with the
// parameter and its moments.  Every sum keeps its order: the results are the hybrid form's bit for bit.
#pragma once
#include "w1_update.h"

namespace aae {

constexpr int kW1RecWords = 24;                                      // one record: 96 bytes
constexpr int kW1OvfRows = 16 * kMB;                                 // rows of a batch of one fused launch
constexpr int kW1OvfWords = 4 + kW1OvfRows / 4 + kW1OvfRows;         // header, rows (bytes), scaled values
static_assert(kW1OvfRows <= 256 && kW1HybRows == 16, "w1_lists.h: a row is one byte, a record holds 16 of them");

struct ItemLists {
    unsigned* rec;          // [cap][kW1RecWords]
    unsigned* ovf;          // [hot_cap][kW1OvfWords]
    int* hot_count;         // overflow slots in use
    int cap, hot_cap;
};
struct ItemListJob {        // piggy-backed on a chain launch when enabled: its LAST nblocks workgroups
    int enabled, nblocks;
    const int* ulist; const int* ucount;
    const int* tstart; const int* eb; const int* en; const float* ev;
    const float* rscale; int rows;
    ItemLists out;
    int* hot_zero;          // the OTHER list set's slot counter (the next build's), zeroed here - the two alternate
};

constexpr int kW1BuildDeferWords = 64;      // deferred items' bitmap of a builder workgroup: (round, wave) pairs
// LDS words of a builder workgroup of `waves` waves
__host__ __device__ inline size_t w1_lists_build_lds_words(int waves) {
    return (size_t)waves * 2 * kW1HybRows + kW1BuildDeferWords + 2 * ((kW1OvfRows + 31) >> 5) + 2 * kW1OvfRows + 4;
}

// one item by the whole workgroup: the bitmap and prefix form of w1_item_update_one, list -> record or overflow slot
template <int NT>
__device__ __forceinline__ void w1_lists_build_one(const ItemListJob& a, unsigned* scratch, int u) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nw = (a.rows + 31) >> 5;
    unsigned* bm = scratch;                                // [nw]   bit b: row b holds the item
    int* pre = reinterpret_cast<int*>(bm + nw);            // [nw]   rows below word w that hold it
    int* rl = pre + nw;                                    // [rows] its rows, ascending
    float* xl = reinterpret_cast<float*>(rl + a.rows);     // [rows] their values
    int* s_n = reinterpret_cast<int*>(xl + a.rows);        // [2]    n, overflow slot
    const int item = a.ulist[u];
    const int tile = item / kTI, it = item - tile * kTI;
    const int e0 = a.tstart[tile], e1 = a.tstart[tile + 1];
    for (int i = tid; i < nw; i += NT) bm[i] = 0u;
    __syncthreads();
    int my_r = -1; float my_x = 0.f;
    {
        const int ec = min(e0 + tid, e1 - 1);              // the first group also keeps its value
        const int en_e = a.en[ec], r = a.eb[ec]; const float x = a.ev[ec];
        if (e0 + tid < e1 && en_e == it) { atomicOr(&bm[r >> 5], 1u << (r & 31)); my_r = r; my_x = x; }
    }
    for (int base = e0 + NT; base < e1; base += NT) {
        const int ec = min(base + tid, e1 - 1);
        const int en_e = a.en[ec], r = a.eb[ec];
        if (base + tid < e1 && en_e == it) atomicOr(&bm[r >> 5], 1u << (r & 31));
    }
    __syncthreads();
    if (wave == 0) {                                       // exclusive prefix of the words' popcounts
        int n = 0;
        for (int base = 0; base < nw; base += 64) {
            const int i = base + lane;
            const int c = i < nw ? __popc(bm[i]) : 0;
            int inc = c;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(inc, o, 64); if (lane >= o) inc += t; }
            if (i < nw) pre[i] = n + inc - c;
            n += __shfl(inc, 63, 64);
        }
        if (lane == 0) {
            s_n[0] = n;
            s_n[1] = n > kW1HybRows ? atomicAdd(a.out.hot_count, 1) : 0;
        }
    }
    __syncthreads();
    if (my_r >= 0) {
        const int k = pre[my_r >> 5] + __popc(bm[my_r >> 5] & ((1u << (my_r & 31)) - 1u));
        rl[k] = my_r; xl[k] = my_x;
    }
    for (int base = e0 + NT; base < e1; base += NT) {      // (hot tiles only)
        const int ec = min(base + tid, e1 - 1);
        const int en_e = a.en[ec], r = a.eb[ec]; const float x = a.ev[ec];
        if (base + tid < e1 && en_e == it) {
            const int k = pre[r >> 5] + __popc(bm[r >> 5] & ((1u << (r & 31)) - 1u));
            rl[k] = r; xl[k] = x;
        }
    }
    __syncthreads();
    const int n = s_n[0], slot = s_n[1];
    unsigned* rec = a.out.rec + (size_t)u * kW1RecWords;
    if (tid == 0) { rec[0] = (unsigned)item; rec[1] = (unsigned)n; rec[2] = (unsigned)slot; }
    if (n <= kW1HybRows) {
        if (tid < n) {
            const int r = rl[tid];
            reinterpret_cast<unsigned char*>(rec + 4)[tid] = (unsigned char)r;
            reinterpret_cast<float*>(rec + 8)[tid] = xl[tid] * a.rscale[r];
        }
    } else if (slot < a.out.hot_cap) {
        unsigned* o = a.out.ovf + (size_t)slot * kW1OvfWords;
        if (tid == 0) { o[0] = (unsigned)item; o[1] = (unsigned)n; }
        for (int i = tid; i < n; i += NT) {
            const int r = rl[i];
            reinterpret_cast<unsigned char*>(o + 4)[i] = (unsigned char)r;
            reinterpret_cast<float*>(o + 4 + kW1OvfRows / 4)[i] = xl[i] * a.rscale[r];
        }
    }
    __syncthreads();                                       // the lists are rewritten next
}

// The builder: NT-thread workgroups, one wave per item (the hybrid form's collection and rank); items with more rows than
// a record holds are noted in an LDS bitmap and taken by the whole workgroup behind a barrier.
template <int NT>
__device__ __forceinline__ void w1_lists_build_body(const ItemListJob& a, unsigned* lds, int vblock, int vgrid) {
    constexpr int NW = NT / 64;
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned* defer = lds + NW * 2 * kW1HybRows;
    unsigned* scratch = defer + kW1BuildDeferWords;
    if (vblock == 0 && tid == 0) *a.hot_zero = 0;
    for (int i = tid; i < kW1BuildDeferWords; i += NT) defer[i] = 0u;
    __syncthreads();
    int* rl = reinterpret_cast<int*>(lds) + wv * 2 * kW1HybRows;       // rows as found
    float* xl = reinterpret_cast<float*>(rl + kW1HybRows);              // their values
    const int cnt = min(*a.ucount, a.out.cap);
    const int ustep = vgrid * NW;
    constexpr int kRounds = kW1BuildDeferWords * 32 / NW;
    int round = 0;
    for (int u = vblock + wv * vgrid; u < cnt && round < kRounds; u += ustep, ++round) {
        const int item = a.ulist[u];
        const int tile = item / kTI, it = item - tile * kTI;
        const int e0 = a.tstart[tile], e1 = a.tstart[tile + 1];
        int n = 0;
        for (int base = e0; base < e1; base += 256) {      // four groups of 64 entries requested together, taken in order
            int en4[4], r4[4]; float x4[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { const int ec = min(base + 64 * j + lane, e1 - 1); en4[j] = a.en[ec]; r4[j] = a.eb[ec]; x4[j] = a.ev[ec]; }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool hit = base + 64 * j + lane < e1 && en4[j] == it;
                const unsigned long long bal = __ballot(hit);
                const int k = n + __popcll(bal & ((1ull << lane) - 1ull));
                if (hit && k < kW1HybRows) { rl[k] = r4[j]; xl[k] = x4[j]; }
                n += __popcll(bal);
            }
        }
        if (n > kW1HybRows) {                           // more rows than a record holds: the whole workgroup takes it below
            const int b = round * NW + wv;
            if (lane == 0) atomicOr(&defer[b >> 5], 1u << (b & 31));
            continue;
        }
        unsigned* rec = a.out.rec + (size_t)u * kW1RecWords;
        if (lane == 0) { rec[0] = (unsigned)item; rec[1] = (unsigned)n; rec[2] = 0u; }
        if (lane < n) {                                 // rank by row (distinct rows: the batch's CSR is canonical)
            const int r = rl[lane];
            int k = 0;
            for (int j = 0; j < n; ++j) k += (rl[j] < r || (rl[j] == r && j < lane)) ? 1 : 0;   // total order: a duplicate (row, item) pair of a non-canonical CSR still gets a slot of its own
            reinterpret_cast<unsigned char*>(rec + 4)[k] = (unsigned char)r;
            reinterpret_cast<float*>(rec + 8)[k] = xl[lane] * a.rscale[r];
        }
    }
    __syncthreads();
    // the deferred items, with all waves
    const int rounds = vblock < cnt ? (cnt - vblock + ustep - 1) / ustep : 0;      // (of wave 0, the one with the most)
    const int nbits = min(rounds, kRounds) * NW;
    for (int b = 0; b < nbits; ++b) {
        if (!((defer[b >> 5] >> (b & 31)) & 1u)) continue;             // (uniform: LDS word read by every thread)
        w1_lists_build_one<NT>(a, scratch, vblock + (b % NW) * vgrid + (b / NW) * ustep);
    }
    // a launch so narrow that the list takes more rounds than the bitmap holds: the rest by the whole workgroup, in order
    for (int u = vblock + kRounds * ustep; u < cnt; u += vgrid) w1_lists_build_one<NT>(a, scratch, u);
}

// ---------------------------------------------------------------------------------------------------------------------
// Consumers (grouped_dw_kernel's first-layer workgroups; fused optimiser only, rows read in place).
// ---------------------------------------------------------------------------------------------------------------------

// Items of up to kW1HybRows rows: one wave per record, no LDS, no barrier.  The sum and the update are w1_item_hybrid_body's.
__device__ __forceinline__ void w1_lists_wave_body(const W1Items& a, const ItemLists& L, int vblock, int vgrid) {
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int ustep = vgrid * 4;
    int u = vblock + wv * vgrid;
    // the record, the count and the optimiser's scalars travel together: the bound is checked behind the load
    unsigned rw = L.rec[(size_t)min(u, L.cap - 1) * kW1RecWords + min(lane, kW1RecWords - 1)];
    const int cnt = min(*a.ucount, L.cap);
    const OptScalars s = *a.sc;
    while (u < cnt) {
        const int item = (int)__builtin_amdgcn_readlane(rw, 0);
        const int n = (int)__builtin_amdgcn_readlane(rw, 1);
        if (n <= kW1HybRows) {
            const int c4 = 4 * lane;
            const size_t o0 = (size_t)item * a.ldw + min(c4, a.ldw - 4);
            float4 pw = *reinterpret_cast<const float4*>(a.W + o0), pm = make_float4(0.f, 0.f, 0.f, 0.f), pv = pm;
            if (!s.is_sgd) { pm = *reinterpret_cast<const float4*>(a.M + o0); pv = *reinterpret_cast<const float4*>(a.V + o0); }
            for (int cb = 0; cb < a.h; cb += 256) {
                const int cc = min(cb + c4, a.ld - 4);
                float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
                constexpr int kU = 8;                   // rows whose loads travel together; the adds stay in row order
                for (int i0 = 0; i0 < n; i0 += kU) {
                    float4 g[kU]; float x[kU];
#pragma unroll
                    for (int j = 0; j < kU; ++j) {
                        const int i = min(i0 + j, n - 1);
                        const int r = (int)((__builtin_amdgcn_readlane(rw, 4 + (i >> 2)) >> (8 * (i & 3))) & 255u);
                        x[j] = i0 + j < n ? __uint_as_float(__builtin_amdgcn_readlane(rw, 8 + i)) : 0.f;
                        g[j] = *reinterpret_cast<const float4*>(a.ga1 + (size_t)r * a.ld + cc);
                    }
#pragma unroll
                    for (int j = 0; j < kU; ++j) {
                        acc.x += x[j] * g[j].x; acc.y += x[j] * g[j].y; acc.z += x[j] * g[j].z; acc.w += x[j] * g[j].w;
                    }
                }
                const int c = cb + c4;
                if (c >= a.h) acc.x = 0.f;              // (columns h .. of a row are padding: a zero gradient)
                if (c + 1 >= a.h) acc.y = 0.f;
                if (c + 2 >= a.h) acc.z = 0.f;
                if (c + 3 >= a.h) acc.w = 0.f;
                const size_t o = (size_t)item * a.ldw + min(c, a.ldw - 4);
                if (cb > 0) {
                    pw = *reinterpret_cast<const float4*>(a.W + o);
                    if (!s.is_sgd) { pm = *reinterpret_cast<const float4*>(a.M + o); pv = *reinterpret_cast<const float4*>(a.V + o); }
                }
                if (c < a.ldw) {
                    adam_update(pw.x, pm.x, pv.x, acc.x, s); adam_update(pw.y, pm.y, pv.y, acc.y, s);
                    adam_update(pw.z, pm.z, pv.z, acc.z, s); adam_update(pw.w, pm.w, pv.w, acc.w, s);
                    *reinterpret_cast<float4*>(a.W + o) = pw;
                    if (!s.is_sgd) { *reinterpret_cast<float4*>(a.M + o) = pm; *reinterpret_cast<float4*>(a.V + o) = pv; }
                }
            }
            if (a.mark_synced && lane == 0) a.tsync[item] = (int)*a.step_ctr;
        }
        u += ustep;
        if (u < cnt) rw = L.rec[(size_t)u * kW1RecWords + min(lane, kW1RecWords - 1)];
    }
}

// Items of more rows, one 256-thread workgroup per overflow slot: the sum of w1_item_update_one - the list cut into four
// contiguous quarters, wave w adds its quarter in row order, the four partial sums added in wave order - from the slot's list.
// LDS: 2 * kW1OvfRows + 4 * 256 words.
__device__ __forceinline__ void w1_lists_hot_body(const W1Items& a, const ItemLists& L, unsigned* lds, int vblock, int vgrid) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int* rl = reinterpret_cast<int*>(lds);                 // [kW1OvfRows] the item's rows, ascending
    float* xl = reinterpret_cast<float*>(rl + kW1OvfRows); // [kW1OvfRows] their scaled values
    float* part = xl + kW1OvfRows;                         // [4][256] the waves' partial sums of a column chunk
    const int hc = min(*L.hot_count, L.hot_cap);
    const OptScalars s = *a.sc;
    for (int k = vblock; k < hc; k += vgrid) {
        const unsigned* o = L.ovf + (size_t)k * kW1OvfWords;
        const int item = (int)o[0], n = min((int)o[1], kW1OvfRows);
        if (tid < kW1OvfRows) {
            rl[tid] = reinterpret_cast<const unsigned char*>(o + 4)[tid];
            xl[tid] = reinterpret_cast<const float*>(o + 4 + kW1OvfRows / 4)[tid];
        }
        // this thread's column of the first chunk
        const size_t o0 = (size_t)item * a.ldw + min(tid, a.ldw - 1);
        float pw = a.W[o0], pm = 0.f, pv = 0.f;
        if (!s.is_sgd) { pm = a.M[o0]; pv = a.V[o0]; }
        __syncthreads();
        // this wave's share of the list
        const int q = n <= 16 ? n : (n + 3) >> 2;
        const int i_lo = min(wave * q, n), i_hi = min(i_lo + q, n);
        for (int cb = 0; cb < a.h; cb += 256) {            // 256-column chunks (one for n_hidden <= 256)
            const int c4 = cb + 4 * lane;                  // the accumulating lanes own 4 consecutive columns
            const int cc = min(c4, a.ld - 4);              // (lanes beyond the row: clamped, masked below)
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            constexpr int kU = 16;                         // rows whose loads travel together; the adds stay in row order
            for (int i0 = i_lo; i0 < i_hi; i0 += kU) {
                float4 g[kU]; float x[kU];
#pragma unroll
                for (int j = 0; j < kU; ++j) {
                    const int i = min(i0 + j, i_hi - 1);
                    const int r = rl[i];
                    x[j] = i0 + j < i_hi ? xl[i] : 0.f;
                    g[j] = *reinterpret_cast<const float4*>(a.ga1 + (size_t)r * a.ld + cc);
                }
#pragma unroll
                for (int j = 0; j < kU; ++j) {
                    acc.x += x[j] * g[j].x; acc.y += x[j] * g[j].y; acc.z += x[j] * g[j].z; acc.w += x[j] * g[j].w;
                }
            }
            if (c4 >= a.h) acc.x = 0.f;
            if (c4 + 1 >= a.h) acc.y = 0.f;
            if (c4 + 2 >= a.h) acc.z = 0.f;
            if (c4 + 3 >= a.h) acc.w = 0.f;
            *reinterpret_cast<float4*>(part + wave * 256 + 4 * lane) = acc;
            __syncthreads();
            const int c = cb + tid;
            const float g = ((part[tid] + part[256 + tid]) + part[512 + tid]) + part[768 + tid];      // wave order
            const size_t oc = (size_t)item * a.ldw + min(c, a.ldw - 1);
            if (cb > 0) {
                pw = a.W[oc];
                if (!s.is_sgd) { pm = a.M[oc]; pv = a.V[oc]; }
            }
            if (c < a.ldw) {
                adam_update(pw, pm, pv, g, s);
                a.W[oc] = pw;
                if (!s.is_sgd) { a.M[oc] = pm; a.V[oc] = pv; }
            }
            __syncthreads();                               // part / the lists are rewritten next
        }
        if (a.mark_synced && tid == 0) a.tsync[item] = (int)*a.step_ctr;
    }
}

}  // namespace aae
