// The VAE's middle off the layer-chain kernel (reference vae.py:115-145): the reparametrisation between the [fc21; fc22] product
// and fc3, and its backward with the KL gradient and the KL sum.  A VAE handle wider than a chain slot (cfg.vae_wide) runs its
// hidden half one launch per layer (gemm_f32.h's products with their epilogues, abi_output_layer.h: vae_*_layers) with these
// two kernels in between.  The arithmetic of a cell is chain_ops.h's (reparam_cell, reparam_bwd_cell), the draws are
// COP_REPARAM's: key ^ stream id, the row of the call + grow0, the code column - a seed gives the same eps on either route.
//
// Both kernels: one wavefront per row, four rows per 256-thread workgroup; a lane owns four consecutive code columns where
// every row it touches starts on 16 bytes (vec: n_code % 4 == 0 and the caller's pointers allow it), else one column at a time.
// No LDS beyond the finishing sum's four wave partials.
#pragma once

namespace aae {

struct VaeReparamFwd {
    const float* mulv; int ldm;            // [rows][2 c]: mu, then logvar
    const float* eps_in; int ldi;          // [rows][c] injected draws, or NULL: the counter generator
    float* veps; int lde;                  // [rows][c] the draws of the call, kept for the backward
    float* zc; int ldzc;                   // the decoder input: z -> columns [0, c)
    float* z_out;                          // [rows][c] (aae_vae_encode's copy for the caller) or NULL
    const float* cond; int cond_inc;       // tail != 0: [rows][cond_inc] -> columns [c, cp) of zc (NULL with cond_inc = 0) ...
    int tail;                              // ... and the constant 1 at column cp (fc3's bias column)
    int rows, c, cp, vec, vec_cond;
    uint64_t seed; const long long* step_ctr; uint32_t stream_id; int grow0;
};

__global__ __launch_bounds__(256) void vae_reparam_fwd_kernel(VaeReparamFwd a) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.rows) return;                         // (a whole wavefront: nothing here meets at a barrier)
    const int c = a.c;
    const float* mu = a.mulv + (size_t)row * a.ldm;
    const float* lv = mu + c;
    const float* ei = a.eps_in ? a.eps_in + (size_t)row * a.ldi : nullptr;
    float* eo = a.veps + (size_t)row * a.lde;
    float* z = a.zc + (size_t)row * a.ldzc;
    float* zo = a.z_out ? a.z_out + (size_t)row * c : nullptr;
    const uint64_t k = rng_key(a.seed, (uint64_t)*a.step_ctr, 0) ^ ((uint64_t)a.stream_id * 0xA0761D6478BD642Full);
    const uint32_t grow = (uint32_t)(row + a.grow0);
    if (a.vec) {
        for (int j = 4 * lane; j < c; j += 256) {
            const float4 m4 = *reinterpret_cast<const float4*>(mu + j), l4 = *reinterpret_cast<const float4*>(lv + j);
            float4 e4;
            if (ei) e4 = *reinterpret_cast<const float4*>(ei + j);
            else e4 = make_float4(draw_gauss(k, grow, j), draw_gauss(k, grow, j + 1), draw_gauss(k, grow, j + 2), draw_gauss(k, grow, j + 3));
            const float4 z4 = make_float4(reparam_cell(m4.x, l4.x, e4.x), reparam_cell(m4.y, l4.y, e4.y),
                                          reparam_cell(m4.z, l4.z, e4.z), reparam_cell(m4.w, l4.w, e4.w));
            *reinterpret_cast<float4*>(eo + j) = e4;
            *reinterpret_cast<float4*>(z + j) = z4;
            if (zo) *reinterpret_cast<float4*>(zo + j) = z4;
        }
    } else {
        for (int j = lane; j < c; j += 64) {
            const float e = ei ? ei[j] : draw_gauss(k, grow, j);
            const float zv = reparam_cell(mu[j], lv[j], e);
            eo[j] = e; z[j] = zv;
            if (zo) zo[j] = zv;
        }
    }
    if (!a.tail) return;
    const int ci = a.cond_inc;
    if (ci > 0) {
        const float* cr = a.cond + (size_t)row * ci;
        if (a.vec_cond) for (int j = 4 * lane; j < ci; j += 256) *reinterpret_cast<float4*>(z + c + j) = *reinterpret_cast<const float4*>(cr + j);
        else for (int j = lane; j < ci; j += 64) z[c + j] = cr[j];
    }
    if (lane == 0) z[a.cp] = 1.f;
}

struct VaeReparamBwd {
    const float* dz; int lddz;             // [rows][>= c] dL/dz (the first c columns of dL/d(decoder input))
    const float* mulv; int ldm;            // [rows][2 c] of the forward
    const float* veps; int lde;            // [rows][c] the forward's draws
    float* gmulv; int ldg;                 // [rows][2 c] out: dL/dmu, then dL/dlogvar
    int rows, c, vec;
    float scale;                           // the step's gradient scale (aae_set_grad_scale) on the KL term
    float* row_kl;                         // [rows] scratch: the rows' KL terms
    unsigned* ticket;                      // one word, zero between launches
    float* loss_out;                       // the KL sum of the batch
};

// The KL sum in a FIXED order (the chain op adds its waves' sums with a float atomicAdd, in the order they arrive): a row's
// term = its lanes' columns ascending, then the wave's butterfly; the workgroup that takes the last ticket adds the rows'
// terms - thread t rows t, t + 256, .. ascending, the wave's butterfly, the four waves in order.  The same inputs give the
// same bits on every run.
__global__ __launch_bounds__(256) void vae_reparam_bwd_kernel(VaeReparamBwd a) {
    __shared__ float red[8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = blockIdx.x * 4 + wave;
    const int c = a.c;
    if (row < a.rows) {
        const float* gz = a.dz + (size_t)row * a.lddz;
        const float* mu = a.mulv + (size_t)row * a.ldm;
        const float* lv = mu + c;
        const float* ep = a.veps + (size_t)row * a.lde;
        float* gm = a.gmulv + (size_t)row * a.ldg;
        float* gl = gm + c;
        float kl = 0.f, unused = 0.f;
        if (a.vec) {
            for (int j = 4 * lane; j < c; j += 256) {
                const float4 g4 = *reinterpret_cast<const float4*>(gz + j), m4 = *reinterpret_cast<const float4*>(mu + j);
                const float4 l4 = *reinterpret_cast<const float4*>(lv + j), e4 = *reinterpret_cast<const float4*>(ep + j);
                float4 om, ol;
                om.x = reparam_bwd_cell(true, g4.x, m4.x, l4.x, 0.f, a.scale, kl); ol.x = reparam_bwd_cell(false, g4.x, m4.x, l4.x, e4.x, a.scale, unused);
                om.y = reparam_bwd_cell(true, g4.y, m4.y, l4.y, 0.f, a.scale, kl); ol.y = reparam_bwd_cell(false, g4.y, m4.y, l4.y, e4.y, a.scale, unused);
                om.z = reparam_bwd_cell(true, g4.z, m4.z, l4.z, 0.f, a.scale, kl); ol.z = reparam_bwd_cell(false, g4.z, m4.z, l4.z, e4.z, a.scale, unused);
                om.w = reparam_bwd_cell(true, g4.w, m4.w, l4.w, 0.f, a.scale, kl); ol.w = reparam_bwd_cell(false, g4.w, m4.w, l4.w, e4.w, a.scale, unused);
                *reinterpret_cast<float4*>(gm + j) = om;
                *reinterpret_cast<float4*>(gl + j) = ol;
            }
        } else {
            for (int j = lane; j < c; j += 64) {
                const float g = gz[j], m = mu[j], l = lv[j];
                gm[j] = reparam_bwd_cell(true, g, m, l, 0.f, a.scale, kl);
                gl[j] = reparam_bwd_cell(false, g, m, l, ep[j], a.scale, unused);
            }
        }
        kl = wave_sum(kl);
        if (lane == 0) a.row_kl[row] = kl;
    }
    // hand-off to the finishing workgroup: the rows' terms are complete and released at agent scope before this workgroup's
    // ticket is drawn; whoever draws the last one acquires and reads them all
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = t == gridDim.x - 1;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        red[4] = last ? 1.f : 0.f;
    }
    __syncthreads();
    if (red[4] == 0.f) return;
    float acc = 0.f;
    for (int r = threadIdx.x; r < a.rows; r += 256) acc += __hip_atomic_load(a.row_kl + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    acc = wave_sum(acc);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        *a.loss_out = ((red[0] + red[1]) + red[2]) + red[3];
        __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (zero again for the next launch)
    }
}

}  // namespace aae
