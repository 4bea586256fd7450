// Entry points of the trainable categorical and embedding-bag conditions and of the CSR helpers (cond_embed.h, cond_bag.h,
// cond_csr.h, kernels.h), and the gather of the constant condition blocks (cond_gather.h).
// (one of the parts of aae_abi.hip's translation unit: included there in order, not on its own)
#pragma once

extern "C" {

// ---- what the entry points of the trainable conditions share (who: the entry point's name) -------------------
static_assert(AAE_CAT_SUM == AAE_BAG_SUM && AAE_CAT_MEAN == AAE_BAG_MEAN_WIDTH, "aae_cat_* hands its reduce to the bag kernels");
static_assert(AAE_BAG_SUM == kBagSum && AAE_BAG_MEAN_WIDTH == kBagMeanWidth && AAE_BAG_MEAN_COUNT == kBagMeanCount &&
              AAE_BAG_MAX_PAD0 == kBagMaxPad0 && AAE_BAG_MAX == kBagMax, "the kernels take the ABI's reduce codes");
#define COND_FAIL(text) return fail(AAE_EINVAL, std::string(who) + ": " + text)

static int cond_shape_check(const char* who, int32_t vocab, int32_t dim, int32_t reduce, int32_t padding_idx) {
    if (vocab < 1) COND_FAIL("vocab must be >= 1");
    if (dim < 1 || dim > kCatMaxDim) COND_FAIL("dim must be within [1, 256]");
    if (reduce < AAE_BAG_SUM || reduce > AAE_BAG_MAX) COND_FAIL("unknown reduce");
    if (padding_idx < -1 || padding_idx >= vocab) COND_FAIL("padding_idx must be -1 or a table row");
    return AAE_OK;
}

static int cond_block_check(const char* who, const int32_t* idx_dev, int32_t rows, int32_t width) {
    if (!idx_dev || rows < 1 || width < 1) COND_FAIL("empty index block");
    if ((int64_t)rows * width > (1 << 22)) COND_FAIL("rows * width > 2^22");
    return AAE_OK;
}

static bool cond_is_max(int32_t reduce) { return reduce == AAE_BAG_MAX_PAD0 || reduce == AAE_BAG_MAX; }

static_assert(AAE_BAG_NORM_INF == kBagNormInf && AAE_BAG_NORM_L1 == kBagNormL1 && AAE_BAG_NORM_L2 == kBagNormL2,
              "the kernels take the ABI's norm codes");

// max_norm as the renorm kernels take it (fp32, as torch's own device kernel holds it)
static int cond_norm_check(const char* who, double max_norm, int32_t norm_type, float* max_norm_f) {
    if (!(max_norm > 0.0) || !((float)max_norm > 0.f)) COND_FAIL("max_norm must be > 0");
    if (norm_type != AAE_BAG_NORM_INF && norm_type != AAE_BAG_NORM_L1 && norm_type != AAE_BAG_NORM_L2)
        COND_FAIL("norm_type must be AAE_BAG_NORM_L1, AAE_BAG_NORM_L2 or AAE_BAG_NORM_INF");
    *max_norm_f = (float)max_norm;
    return AAE_OK;
}

// What an update's launches take: the table side of the gradient kernels and dense Adam's scalars.
struct CondUpdate { BagTable a; OptScalars adam; };

// An update in front of its launches: the operand, optimiser and step checks, then the bias corrections into both optimisers' terms.
static int cond_update_begin(const char* who, CondUpdate& u, float* table_dev, float* exp_avg_dev, float* exp_avg_sq_dev,
                             float* grad_scratch_dev, int32_t vocab, int32_t dim, int32_t reduce, int32_t padding_idx,
                             const float* dout_dev, int64_t dout_ld, int32_t optimizer, double lr, int64_t step, int32_t flags) {
    if (flags & ~AAE_BAG_SCALE_BY_FREQ) COND_FAIL("unknown flags");
    if ((flags & AAE_BAG_SCALE_BY_FREQ) && optimizer == AAE_CAT_SPARSE_ADAM)
        COND_FAIL("AAE_BAG_SCALE_BY_FREQ goes with AAE_CAT_ADAM only (torch has no sparse gradient scaled by frequency)");
    if (!table_dev || !exp_avg_dev || !exp_avg_sq_dev || !dout_dev || dout_ld < dim) COND_FAIL("table/state/dout is NULL or dout_ld < dim");
    if (optimizer != AAE_CAT_SPARSE_ADAM && optimizer != AAE_CAT_ADAM) COND_FAIL("unknown optimizer");
    const bool scratch = optimizer == AAE_CAT_ADAM || cond_is_max(reduce);
    if (scratch && !grad_scratch_dev) COND_FAIL("dense Adam and the max modes need grad_scratch_dev");
    if (step < 1) COND_FAIL("step counts from 1");
    const double bc1 = 1.0 - pow(0.9, (double)step), bc2 = 1.0 - pow(0.999, (double)step);
    BagTable& a = u.a;
    a.table = table_dev; a.m = exp_avg_dev; a.v = exp_avg_sq_dev;
    a.gdense = scratch ? grad_scratch_dev : nullptr;
    a.d = dout_dev; a.ldd = dout_ld; a.vocab = vocab; a.dim = dim; a.reduce = reduce; a.pad = padding_idx;
    a.neg_step_size = (float)(-(lr * sqrt(bc2) / bc1));
    a.by_freq = (flags & AAE_BAG_SCALE_BY_FREQ) != 0;
    OptScalars& sc = u.adam;
    memset(&sc, 0, sizeof(sc));
    sc.t = step; sc.neg_step_size = (float)(-(lr / bc1)); sc.bc2_sqrt = (float)sqrt(bc2); sc.lr = lr;
    sc.inv_bc2_sqrt = 1.0f / sc.bc2_sqrt;
    return AAE_OK;
}

// torch.optim.Adam over the whole table from the gradient scratch the update launch filled
static int cond_dense_adam(const CondUpdate& u, hipStream_t s) {
    const BagTable& a = u.a;
    const size_t total = (size_t)a.vocab * a.dim;
    hipLaunchKernelGGL(cat_dense_adam_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a.table, a.m, a.v, a.gdense,
                       total, u.adam);
    LAUNCHCHK("cond_dense_adam");
    return AAE_OK;
}

// ---- padded index blocks (cond_bag.h): EmbeddingBagCondition and CategoricalCondition; aae_cat_* is sum / mean at padding row 0
static int bag_padded_encode(const char* who, const float* table_dev, int32_t vocab, int32_t dim, const int32_t* idx_dev,
                             int32_t rows, int32_t width, int32_t reduce, int32_t padding_idx, float* out_dev, int64_t out_ld,
                             void* stream) {
    TRY(cond_shape_check(who, vocab, dim, reduce, padding_idx));
    TRY(cond_block_check(who, idx_dev, rows, width));
    if (!table_dev || !out_dev || out_ld < dim) COND_FAIL("table/out is NULL or out_ld < dim");
    hipLaunchKernelGGL(bag_encode_kernel, dim3(rows, (dim + 63) / 64), dim3(64), 0, S(stream), table_dev, vocab, dim,
                       idx_dev, width, reduce, padding_idx, out_dev, (long long)out_ld);
    LAUNCHCHK("bag_encode");
    return AAE_OK;
}

static int bag_padded_update(const char* who, float* table_dev, float* exp_avg_dev, float* exp_avg_sq_dev, float* grad_scratch_dev,
                             int32_t vocab, int32_t dim, const int32_t* idx_dev, int32_t rows, int32_t width, int32_t reduce,
                             int32_t padding_idx, const float* dout_dev, int64_t dout_ld, int32_t optimizer, double lr,
                             int64_t step, int32_t flags, void* stream) {
    TRY(cond_shape_check(who, vocab, dim, reduce, padding_idx));
    TRY(cond_block_check(who, idx_dev, rows, width));
    CondUpdate u;
    TRY(cond_update_begin(who, u, table_dev, exp_avg_dev, exp_avg_sq_dev, grad_scratch_dev, vocab, dim, reduce, padding_idx, dout_dev,
                          dout_ld, optimizer, lr, step, flags));
    const BagPadded src = {idx_dev, rows, width};
    const int n = rows * width;
    const dim3 grid((n + kCatWaves - 1) / kCatWaves), block(64 * kCatWaves);
    hipLaunchKernelGGL(bag_update_kernel, grid, block, 0, S(stream), u.a, src);
    LAUNCHCHK("bag_update");
    if (optimizer == AAE_CAT_ADAM) return cond_dense_adam(u, S(stream));
    if (cond_is_max(reduce)) {
        hipLaunchKernelGGL(bag_apply_kernel, grid, block, 0, S(stream), u.a, src);
        LAUNCHCHK("bag_apply");
    }
    return AAE_OK;
}

int aae_cat_encode(const float* table_dev, int32_t vocab, int32_t dim, const int32_t* idx_dev, int32_t rows,
                   int32_t width, int32_t reduce, float* out_dev, int64_t out_ld, void* stream) {
    if (reduce != AAE_CAT_SUM && reduce != AAE_CAT_MEAN) return fail(AAE_EINVAL, "aae_cat_encode: reduce must be sum or mean");
    return bag_padded_encode("aae_cat_encode", table_dev, vocab, dim, idx_dev, rows, width, reduce, 0, out_dev, out_ld, stream);
}

int aae_cat_update(float* table_dev, float* exp_avg_dev, float* exp_avg_sq_dev, float* grad_scratch_dev, int32_t vocab,
                   int32_t dim, const int32_t* idx_dev, int32_t rows, int32_t width, int32_t reduce,
                   const float* dout_dev, int64_t dout_ld, int32_t optimizer, double lr, int64_t step, void* stream) {
    if (reduce != AAE_CAT_SUM && reduce != AAE_CAT_MEAN) return fail(AAE_EINVAL, "aae_cat_update: reduce must be sum or mean");
    return bag_padded_update("aae_cat_update", table_dev, exp_avg_dev, exp_avg_sq_dev, grad_scratch_dev, vocab, dim, idx_dev, rows,
                             width, reduce, 0, dout_dev, dout_ld, optimizer, lr, step, 0, stream);
}

int aae_bag_encode(const float* table_dev, int32_t vocab, int32_t dim, const int32_t* idx_dev, int32_t rows,
                   int32_t width, int32_t reduce, int32_t padding_idx, float* out_dev, int64_t out_ld, void* stream) {
    return bag_padded_encode("aae_bag_encode", table_dev, vocab, dim, idx_dev, rows, width, reduce, padding_idx, out_dev, out_ld,
                             stream);
}

int aae_bag_update_flags(float* table_dev, float* exp_avg_dev, float* exp_avg_sq_dev, float* grad_scratch_dev, int32_t vocab,
                         int32_t dim, const int32_t* idx_dev, int32_t rows, int32_t width, int32_t reduce, int32_t padding_idx,
                         const float* dout_dev, int64_t dout_ld, int32_t optimizer, double lr, int64_t step, int32_t flags,
                         void* stream) {
    return bag_padded_update("aae_bag_update", table_dev, exp_avg_dev, exp_avg_sq_dev, grad_scratch_dev, vocab, dim, idx_dev, rows,
                             width, reduce, padding_idx, dout_dev, dout_ld, optimizer, lr, step, flags, stream);
}

int aae_bag_update(float* table_dev, float* exp_avg_dev, float* exp_avg_sq_dev, float* grad_scratch_dev, int32_t vocab,
                   int32_t dim, const int32_t* idx_dev, int32_t rows, int32_t width, int32_t reduce, int32_t padding_idx,
                   const float* dout_dev, int64_t dout_ld, int32_t optimizer, double lr, int64_t step, void* stream) {
    return aae_bag_update_flags(table_dev, exp_avg_dev, exp_avg_sq_dev, grad_scratch_dev, vocab, dim, idx_dev, rows, width, reduce,
                                padding_idx, dout_dev, dout_ld, optimizer, lr, step, 0, stream);
}

int aae_bag_renorm(float* table_dev, int32_t vocab, int32_t dim, const int32_t* idx_dev, int32_t rows, int32_t width,
                   double max_norm, int32_t norm_type, void* stream) {
    const char* who = "aae_bag_renorm";
    float mn;
    TRY(cond_shape_check(who, vocab, dim, AAE_BAG_SUM, -1));
    TRY(cond_norm_check(who, max_norm, norm_type, &mn));
    TRY(cond_block_check(who, idx_dev, rows, width));
    if (!table_dev) COND_FAIL("table_dev is NULL");
    const BagPadded src = {idx_dev, rows, width};
    const int n = rows * width;
    hipLaunchKernelGGL(bag_renorm_kernel, dim3((n + kCatWaves - 1) / kCatWaves), dim3(64 * kCatWaves), 0, S(stream), table_dev,
                       vocab, dim, src, mn, norm_type);
    LAUNCHCHK("bag_renorm");
    return AAE_OK;
}

// ---- the same bags from a resident CSR (cond_csr.h) ----------------------------------------------------------
// scratch: two key buffers of max_entries, then the int32 arrays hdr[16], off[max_rows + 1], live[max_rows],
// rowof[max_entries], win[max_rows][256]; rounded up to 256 bytes
static int64_t bag_csr_bytes(int64_t max_rows, int64_t max_entries) {
    const int64_t ints = 16 + (max_rows + 1) + max_rows + max_entries + max_rows * kCatMaxDim;
    return (16 * max_entries + 4 * ints + 255) / 256 * 256;
}

int aae_bag_csr_scratch_bytes(int64_t max_rows, int64_t max_entries, int64_t* bytes_out) {
    if (!bytes_out) return fail(AAE_EINVAL, "aae_bag_csr_scratch_bytes: bytes_out is NULL");
    if (max_rows < 0 || max_entries < 0) return fail(AAE_EINVAL, "aae_bag_csr_scratch_bytes: max_rows and max_entries must be >= 0");
    if (max_rows > INT32_MAX || max_entries > INT32_MAX)
        return fail(AAE_EINVAL, "aae_bag_csr_scratch_bytes: max_rows and max_entries must fit an int32");
    *bytes_out = bag_csr_bytes(max_rows, max_entries);
    return AAE_OK;
}

static void bag_csr_carve(BagCsr& c, void* scratch_dev, int32_t rows, int64_t max_entries) {
    c.keys_a = (unsigned long long*)scratch_dev;
    c.keys_b = c.keys_a + max_entries;
    c.hdr = (int*)(c.keys_b + max_entries);
    c.off = c.hdr + 16;
    c.live = c.off + rows + 1;
    c.rowof = c.live + rows;
    c.win = c.rowof + max_entries;
    c.max_entries = (int)max_entries;
}

// the checks of both calls; fills c
static int bag_csr_check(const char* who, BagCsr& c, int32_t vocab, int32_t dim, const int64_t* indptr_dev,
                         const int32_t* indices_dev, const float* weights_dev, int64_t n_docs, int64_t nnz,
                         const int32_t* row_ids_dev, int64_t row0, int32_t rows, int64_t max_entries, int32_t reduce,
                         int32_t padding_idx, void* scratch_dev, int64_t scratch_bytes) {
    TRY(cond_shape_check(who, vocab, dim, reduce, padding_idx));
    if (rows < 1) COND_FAIL("rows must be >= 1");
    if (!indptr_dev || !indices_dev) COND_FAIL("indptr_dev / indices_dev is NULL");
    if (n_docs < 1 || nnz < 0) COND_FAIL("need n_docs >= 1 and nnz >= 0");
    if (!row_ids_dev && (row0 < 0 || row0 + rows > n_docs)) COND_FAIL("row0 .. row0 + rows is not inside [0, n_docs)");
    if (max_entries < 0) COND_FAIL("max_entries must be >= 0");
    if (max_entries > kBagCsrMaxEntries) COND_FAIL("max_entries: a step takes at most 2^22 entries");
    if (weights_dev && reduce != AAE_BAG_SUM) COND_FAIL("weights_dev goes with reduce AAE_BAG_SUM only");
    if (!scratch_dev || ((uintptr_t)scratch_dev & 7)) COND_FAIL("scratch_dev is NULL or not 8-byte aligned");
    if (scratch_bytes < bag_csr_bytes(rows, max_entries)) COND_FAIL("scratch_bytes is smaller than aae_bag_csr_scratch_bytes(rows, max_entries)");
    c.indptr = (const long long*)indptr_dev; c.indices = indices_dev; c.weights = weights_dev;
    c.n_docs = n_docs; c.nnz = nnz; c.row_ids = row_ids_dev; c.row0 = row0; c.rows = rows;
    bag_csr_carve(c, scratch_dev, rows, max_entries);
    return AAE_OK;
}

// The step's entries as keys grouped by table row under the padding row `pad` (cond_csr.h): row scan, LDS sort, merge passes up
// to the entry bound (E itself stays on the device).  Returns the buffer the sorted keys end in (keys_a or keys_b).
static const unsigned long long* bag_csr_sorted(const BagCsr& c, int32_t vocab, int32_t pad, int64_t max_entries, hipStream_t s) {
    hipLaunchKernelGGL(bagcsr_rowinfo_kernel, dim3(1), dim3(kBagCsrScanNT), 0, s, c);
    hipLaunchKernelGGL(bagcsr_sort_kernel, dim3((unsigned)((max_entries + kBagCsrSort - 1) / kBagCsrSort)), dim3(kBagCsrNT), 0, s, c,
                       vocab, pad);
    unsigned long long *src = c.keys_a, *dst = c.keys_b;
    for (int64_t w = kBagCsrSort; w < max_entries; w <<= 1) {
        hipLaunchKernelGGL(bagcsr_merge_kernel, dim3((unsigned)((max_entries + kBagCsrNT - 1) / kBagCsrNT)), dim3(kBagCsrNT), 0, s,
                           src, dst, c.hdr, (int)w);
        unsigned long long* t = src; src = dst; dst = t;
    }
    return src;
}

// the update launch's grid: a wavefront per sorted position, grid-stride beyond kBagCsrMaxGrid workgroups
static dim3 bag_csr_grid(int64_t max_entries) {
    const int64_t want = (max_entries + kCatWaves - 1) / kCatWaves;
    return dim3((unsigned)(want < kBagCsrMaxGrid ? want : kBagCsrMaxGrid));
}

int aae_bag_csr_encode(const float* table_dev, int32_t vocab, int32_t dim, const int64_t* indptr_dev,
                       const int32_t* indices_dev, const float* weights_dev, int64_t n_docs, int64_t nnz,
                       const int32_t* row_ids_dev, int64_t row0, int32_t rows, int32_t reduce, int32_t padding_idx,
                       float* out_dev, int64_t out_ld, void* scratch_dev, int64_t scratch_bytes, void* stream) {
    BagCsr c;
    TRY(bag_csr_check("aae_bag_csr_encode", c, vocab, dim, indptr_dev, indices_dev, weights_dev, n_docs, nnz, row_ids_dev, row0,
                      rows, 0, reduce, padding_idx, scratch_dev, scratch_bytes));
    if (!table_dev || !out_dev || out_ld < dim) return fail(AAE_EINVAL, "aae_bag_csr_encode: table_dev / out_dev is NULL or out_ld < dim");
    if (reduce == AAE_BAG_MEAN_WIDTH || reduce == AAE_BAG_MAX_PAD0) {        // the two modes that see the width
        hipLaunchKernelGGL(bagcsr_rowinfo_kernel, dim3(1), dim3(kBagCsrScanNT), 0, S(stream), c);
        LAUNCHCHK("bagcsr_rowinfo");
    }
    hipLaunchKernelGGL(bagcsr_encode_kernel, dim3(rows, (dim + 63) / 64), dim3(64), 0, S(stream), c, table_dev, vocab, dim,
                       reduce, padding_idx, out_dev, (long long)out_ld);
    LAUNCHCHK("bagcsr_encode");
    return AAE_OK;
}

int aae_bag_csr_update_flags(float* table_dev, float* exp_avg_dev, float* exp_avg_sq_dev, float* grad_scratch_dev, int32_t vocab,
                             int32_t dim, const int64_t* indptr_dev, const int32_t* indices_dev, const float* weights_dev,
                             int64_t n_docs, int64_t nnz, const int32_t* row_ids_dev, int64_t row0, int32_t rows,
                             int64_t max_entries, int32_t reduce, int32_t padding_idx, const float* dout_dev, int64_t dout_ld,
                             int32_t optimizer, double lr, int64_t step, int32_t flags, void* scratch_dev,
                             int64_t scratch_bytes, void* stream) {
    BagCsr c;
    TRY(bag_csr_check("aae_bag_csr_update", c, vocab, dim, indptr_dev, indices_dev, weights_dev, n_docs, nnz, row_ids_dev, row0,
                      rows, max_entries, reduce, padding_idx, scratch_dev, scratch_bytes));
    if (max_entries < 1) return fail(AAE_EINVAL, "aae_bag_csr_update: max_entries must be >= 1");
    CondUpdate u;
    TRY(cond_update_begin("aae_bag_csr_update", u, table_dev, exp_avg_dev, exp_avg_sq_dev, grad_scratch_dev, vocab, dim, reduce,
                          padding_idx, dout_dev, dout_ld, optimizer, lr, step, flags));
    hipStream_t s = S(stream);
    const unsigned long long* src = bag_csr_sorted(c, vocab, padding_idx, max_entries, s);
    if (reduce >= AAE_BAG_MEAN_COUNT)
        hipLaunchKernelGGL(bagcsr_rowpass_kernel, dim3(rows, reduce == AAE_BAG_MEAN_COUNT ? 1 : (dim + 63) / 64), dim3(64), 0, s, c,
                           table_dev, vocab, dim, reduce, padding_idx);
    const dim3 grid = bag_csr_grid(max_entries), block(64 * kCatWaves);
    hipLaunchKernelGGL(bagcsr_update_kernel, grid, block, 0, s, u.a, c, src, 0);
    LAUNCHCHK("bagcsr_update");
    if (optimizer == AAE_CAT_ADAM) return cond_dense_adam(u, s);
    if (cond_is_max(reduce)) {          // SparseAdam of the max modes: the owners apply their row from the scratch and clear it
        hipLaunchKernelGGL(bagcsr_update_kernel, grid, block, 0, s, u.a, c, src, 1);
        LAUNCHCHK("bagcsr_apply");
    }
    return AAE_OK;
}

int aae_bag_csr_update(float* table_dev, float* exp_avg_dev, float* exp_avg_sq_dev, float* grad_scratch_dev, int32_t vocab,
                       int32_t dim, const int64_t* indptr_dev, const int32_t* indices_dev, const float* weights_dev,
                       int64_t n_docs, int64_t nnz, const int32_t* row_ids_dev, int64_t row0, int32_t rows,
                       int64_t max_entries, int32_t reduce, int32_t padding_idx, const float* dout_dev, int64_t dout_ld,
                       int32_t optimizer, double lr, int64_t step, void* scratch_dev, int64_t scratch_bytes, void* stream) {
    return aae_bag_csr_update_flags(table_dev, exp_avg_dev, exp_avg_sq_dev, grad_scratch_dev, vocab, dim, indptr_dev, indices_dev,
                                    weights_dev, n_docs, nnz, row_ids_dev, row0, rows, max_entries, reduce, padding_idx, dout_dev,
                                    dout_ld, optimizer, lr, step, 0, scratch_dev, scratch_bytes, stream);
}

int aae_bag_csr_renorm(float* table_dev, int32_t vocab, int32_t dim, const int64_t* indptr_dev, const int32_t* indices_dev,
                       int64_t n_docs, int64_t nnz, const int32_t* row_ids_dev, int64_t row0, int32_t rows, int64_t max_entries,
                       double max_norm, int32_t norm_type, void* scratch_dev, int64_t scratch_bytes, void* stream) {
    const char* who = "aae_bag_csr_renorm";
    float mn;
    TRY(cond_norm_check(who, max_norm, norm_type, &mn));
    BagCsr c;
    TRY(bag_csr_check(who, c, vocab, dim, indptr_dev, indices_dev, nullptr, n_docs, nnz, row_ids_dev, row0, rows, max_entries,
                      AAE_BAG_SUM, -1, scratch_dev, scratch_bytes));
    if (max_entries < 1) COND_FAIL("max_entries must be >= 1");
    if (!table_dev) COND_FAIL("table_dev is NULL");
    hipStream_t s = S(stream);
    const unsigned long long* src = bag_csr_sorted(c, vocab, -1, max_entries, s);       // no padding row: every named row has an owner
    hipLaunchKernelGGL(bagcsr_renorm_kernel, bag_csr_grid(max_entries), dim3(64 * kCatWaves), 0, s, table_dev, dim, c, src, mn,
                       norm_type);
    LAUNCHCHK("bagcsr_renorm");
    return AAE_OK;
}

#undef COND_FAIL

int aae_csr_embed(const int64_t* indptr_dev, const int32_t* indices_dev, const float* values_dev, int32_t n_rows,
                  const float* table_dev, int32_t n_table_rows, int32_t dim, int64_t table_ld, float* out_dev,
                  int64_t out_ld, void* stream) {
    if (!indptr_dev || !table_dev || !out_dev) return fail(AAE_EINVAL, "aae_csr_embed: indptr/table/out is NULL");
    if (n_rows < 0 || n_table_rows < 1 || dim < 1 || table_ld < dim || out_ld < dim)
        return fail(AAE_EINVAL, "aae_csr_embed: bad shape (need n_table_rows >= 1, dim >= 1, leading dimensions >= dim)");
    if (n_rows == 0) return AAE_OK;
    if (!indices_dev || !values_dev) return fail(AAE_EINVAL, "aae_csr_embed: indices/values is NULL");
    hipLaunchKernelGGL(csr_embed_kernel, dim3(n_rows), dim3(256), 0, S(stream), (const long long*)indptr_dev, indices_dev,
                       values_dev, table_dev, n_table_rows, dim, (long long)table_ld, out_dev, (long long)out_ld);
    LAUNCHCHK("csr_embed");
    return AAE_OK;
}

// ---- constant condition blocks resident in HBM (cond_gather.h) ------------------------------------------------
static_assert(AAE_COND_SRC_MAX == kCondSrcMax, "the kernel's argument block holds the ABI's number of sources");

int aae_cond_gather(const aae_cond_src* srcs, int32_t n_srcs, const int32_t* row_ids_dev, int64_t row0, int32_t rows,
                    float* out_dev, int64_t out_ld, void* stream) {
    const char* who = "aae_cond_gather";
#define COND_FAIL(text) return fail(AAE_EINVAL, std::string(who) + ": " + text)
    if (!srcs || !out_dev) COND_FAIL("srcs / out_dev is NULL");
    if (n_srcs < 1 || n_srcs > AAE_COND_SRC_MAX) COND_FAIL("n_srcs must be within [1, AAE_COND_SRC_MAX]");
    if (rows < 0) COND_FAIL("rows must be >= 0");
    CondGatherArgs a;
    memset(&a, 0, sizeof(a));
    // 16-byte loads and stores where both sides allow them: the output's part of the rule is the call's, the rest a source's
    const bool out16 = ((uintptr_t)out_dev & 15) == 0 && out_ld % 4 == 0;
    for (int i = 0; i < n_srcs; ++i) {
        const aae_cond_src& s = srcs[i];
        if (!s.base_dev) COND_FAIL("a source's base_dev is NULL");
        if (s.width < 1) COND_FAIL("a source's width must be >= 1");
        if (s.ld < s.width) COND_FAIL("a source's ld is smaller than its width");
        if (s.n_docs < 0) COND_FAIL("a source's n_docs must be >= 0");
        if (s.col0 < 0) COND_FAIL("a source's col0 must be >= 0");
        if ((int64_t)s.col0 + s.width > out_ld) COND_FAIL("a source's col0 + width passes out_ld");
        const bool vec = out16 && ((uintptr_t)s.base_dev & 15) == 0 && s.ld % 4 == 0 && s.col0 % 4 == 0;
        a.src[i] = {reinterpret_cast<const unsigned*>(s.base_dev), (long long)s.ld, (long long)s.n_docs, s.width, s.col0,
                    vec ? s.width / 4 : 0, 0};
    }
#undef COND_FAIL
    if (rows == 0) return AAE_OK;
    a.row_ids = row_ids_dev; a.row0 = row0; a.out = reinterpret_cast<unsigned*>(out_dev); a.out_ld = out_ld; a.rows = rows;
    hipLaunchKernelGGL(pick_cond_gather(), dim3((unsigned)(((int64_t)rows + kCondGatherWaves - 1) / kCondGatherWaves), (unsigned)n_srcs),
                       dim3(64, kCondGatherWaves), 0, S(stream), a);
    LAUNCHCHK("cond_gather");
    return AAE_OK;
}

int aae_dense_to_csr(const void* dense_dev, int32_t elem_bytes, int64_t ld, int32_t rows, int32_t n_cols,
                     int64_t* indptr_dev, int32_t* indices_dev, float* values_dev, int64_t capacity,
                     int32_t* scratch_dev, int32_t* stats_out_host, void* stream) {
    if (!dense_dev || !indptr_dev || !indices_dev || !values_dev || !scratch_dev || !stats_out_host)
        return fail(AAE_EINVAL, "aae_dense_to_csr: NULL argument");
    if (rows < 1 || n_cols < 1 || ld < n_cols || capacity < 1) return fail(AAE_EINVAL, "aae_dense_to_csr: bad shape");
    if (elem_bytes != 4 && elem_bytes != 8) return fail(AAE_EINVAL, "aae_dense_to_csr: elem_bytes must be 4 (float32) or 8 (float64)");
    hipStream_t s = S(stream);
    int* stats = scratch_dev;                 // [0..3] statistics, [8..] row counts
    int* rowcnt = scratch_dev + 8;
    HIPCHK(hipMemsetAsync(stats, 0, 8 * sizeof(int), s));
    if (elem_bytes == 4) hipLaunchKernelGGL(dense_count_kernel<float>, dim3(rows), dim3(256), 0, s, (const float*)dense_dev, (long long)ld, n_cols, rowcnt, stats);
    else hipLaunchKernelGGL(dense_count_kernel<double>, dim3(rows), dim3(256), 0, s, (const double*)dense_dev, (long long)ld, n_cols, rowcnt, stats);
    hipLaunchKernelGGL(dense_scan_kernel, dim3(1), dim3(1024), 0, s, rowcnt, rows, (long long)capacity, (long long*)indptr_dev, stats);
    if (elem_bytes == 4) hipLaunchKernelGGL(dense_fill_kernel<float>, dim3(rows), dim3(256), 0, s, (const float*)dense_dev, (long long)ld, n_cols, (const long long*)indptr_dev, stats, indices_dev, values_dev);
    else hipLaunchKernelGGL(dense_fill_kernel<double>, dim3(rows), dim3(256), 0, s, (const double*)dense_dev, (long long)ld, n_cols, (const long long*)indptr_dev, stats, indices_dev, values_dev);
    LAUNCHCHK("dense_to_csr");
    HIPCHK(hipMemcpyAsync(stats_out_host, stats, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return AAE_OK;
}


}  // extern "C"
