// DenoisingAutoEncoder's corruption from the device generator: the entry points (kernels: dae_corrupt.h).
// (one of the parts of aae_abi.hip's translation unit: included there in order, not on its own)
#pragma once

// The dense branch of ae_encode_impl (abi_step_open.h) with a pending aae_set_input_noise_gen: Xn = batch + scale x the stream-14
// draws of the OPENED step (advance_step_kernel ran in front on this stream: *step_ctr holds the value slab_reduce_fwd_kernel
// reads two launches later), written once; no noise matrix exists in memory.
static int launch_dense_noise_gen(aae_model* m, float scale, hipStream_t s) {
    const int rows = m->rows, ldx = m->ldn;
    // ~2048 workgroups of four waves (eight a CU), at most kDaeChunksMax chunks a row, whole 256-column strides a chunk
    int chunks = std::max(1, std::min(kDaeChunksMax, (2048 + rows - 1) / rows));
    const int cc = ((ldx + chunks - 1) / chunks + 255) & ~255;
    chunks = (ldx + cc - 1) / cc;
    const int normalize = (int)m->cfg.normalize_inputs;
    hipLaunchKernelGGL(dense_noise_gen_kernel, dim3(chunks, rows), dim3(256), 0, s, m->bv, scale, m->N, normalize, cc, m->rng_row0,
                       (uint64_t)m->cfg.seed, (const long long*)m->step_ctr, m->Xn.p, ldx, m->noise_l1);
    LAUNCHCHK("dense_noise_gen");
    if (normalize) {
        hipLaunchKernelGGL(dense_noise_finish_kernel, dim3(chunks, rows), dim3(256), 0, s, m->bv, scale, m->N, cc, m->rng_row0,
                           (uint64_t)m->cfg.seed, (const long long*)m->step_ctr, m->Xn.p, ldx, (const float*)m->noise_l1);
        LAUNCHCHK("dense_noise_finish");
    }
    return AAE_OK;
}

extern "C" {

int aae_dae_thin(aae_handle h, const int64_t* indptr_dev, const int32_t* indices_dev, const float* values_dev, int64_t n_rows,
                 float p, float* out_values_dev, void* stream) {
    if (!h) return fail(AAE_EINVAL, "handle is NULL");
    if (h->cfg.rng_mode != AAE_RNG_DEVICE) return fail(AAE_ESTATE, "aae_dae_thin draws from the device generator: the handle is not in rng_mode device");
    if (!indptr_dev || !indices_dev || !values_dev || !out_values_dev) return fail(AAE_EINVAL, "aae_dae_thin: NULL array");
    if (n_rows < 0 || n_rows > 0x7FFFFFFF) return fail(AAE_EINVAL, "aae_dae_thin: n_rows outside [0, 2^31)");
    if (!(p >= 0.f && p <= 1.f)) return fail(AAE_EINVAL, "aae_dae_thin: p (the drop probability) outside [0, 1]");
    if (n_rows == 0) return AAE_OK;
    const int enabled = p > 0.f ? 1 : 0;                      // p == 0 keeps everything without comparing a word
    if (!enabled && out_values_dev == values_dev) return AAE_OK;
    const uint32_t thr = (uint32_t)std::min(4294967295.0, (double)p * 4294967296.0);      // make_drop's threshold
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((n_rows + 3) / 4, 2048));
    hipLaunchKernelGGL(dae_thin_kernel, dim3(grid), dim3(256), 0, S(stream), indptr_dev, indices_dev, values_dev, n_rows, thr, enabled,
                       (uint64_t)h->cfg.seed, (const long long*)h->step_ctr, out_values_dev);
    LAUNCHCHK("dae_thin");
    return AAE_OK;
}

int aae_set_input_noise_gen(aae_handle h, float scale) {
    if (!h) return fail(AAE_EINVAL, "handle is NULL");
    if (!h->Xn.p) return fail(AAE_ESTATE, "aae_set_input_noise_gen: the model was not created with cfg.dense_noise = 1");
    if (h->cfg.rng_mode != AAE_RNG_DEVICE) return fail(AAE_ESTATE, "aae_set_input_noise_gen draws from the device generator: the handle is not in rng_mode device");
    if (!(scale == scale) || fabsf(scale) > 3.0e38f) return fail(AAE_EINVAL, "aae_set_input_noise_gen: scale is not finite");
    h->noise_next = nullptr; h->noise_ld = 0;                 // (the later call wins)
    h->noise_gen_next = true; h->noise_gen_scale = scale;
    return AAE_OK;
}

}  // extern "C"
