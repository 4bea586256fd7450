// A batch's rows of the constant condition blocks (PretrainedWordEmbeddingCondition: one fp32 [n_docs, width] matrix per
// block, resident in HBM) copied into the step's condition block at their column offsets: aae_cond_gather.  One launch for
// up to kCondSrcMax blocks - what three index_selects and a cat do for MPD's condition list.  A copy: the words travel as
// unsigned integers, so NaN payloads and -0.0 arrive as they are.
#pragma once
#include "device_common.h"

namespace aae {

constexpr int kCondSrcMax = 8;        // AAE_COND_SRC_MAX: blocks of one call
constexpr int kCondGatherWaves = 4;   // wavefronts per workgroup, a row of the batch each

// One block.  quads: the 16-byte pieces of a row that go as one load and one store - width / 4 where base, ld, the output
// block, out_ld and col0 keep every row of both sides on 16 bytes (the entry point decides, per block), else 0: the scalar
// path.  The columns behind the last quad go one at a time either way, so no load leaves a row's [0, width).
struct CondGatherSrc { const unsigned* base; long long ld; long long n_docs; int width; int col0; int quads; int pad_; };
struct CondGatherArgs {
    CondGatherSrc src[kCondSrcMax];
    const int* row_ids;               // [rows] on the device, or nullptr: the rows row0 .. row0 + rows
    long long row0;
    unsigned* out;
    long long out_ld;
    int rows;
};

// grid (ceil(rows / kCondGatherWaves), blocks), block (64, kCondGatherWaves): a wavefront copies one row of one block, its
// lanes striding over the row's quads, then over the columns that are left.  A row id outside [0, n_docs) gives a row of zeros
// (the bag CSR's rule: an empty row) and reads nothing.  Every offset is 64-bit: id * ld passes 2^31 at a few million documents.
__global__ void __launch_bounds__(64 * kCondGatherWaves)
cond_gather_kernel(CondGatherArgs a) {
    const CondGatherSrc& s = a.src[blockIdx.y];
    const int r = blockIdx.x * kCondGatherWaves + threadIdx.y;
    if (r >= a.rows) return;
    const long long id = a.row_ids ? (long long)a.row_ids[r] : a.row0 + r;
    const bool live = id >= 0 && id < s.n_docs;
    const unsigned* in = s.base + (live ? id : 0) * s.ld;
    unsigned* out = a.out + (long long)r * a.out_ld + s.col0;
    const int nq = s.quads;
    for (int q = threadIdx.x; q < nq; q += 64)
        reinterpret_cast<uint4*>(out)[q] = live ? reinterpret_cast<const uint4*>(in)[q] : make_uint4(0u, 0u, 0u, 0u);
    for (int c = 4 * nq + threadIdx.x; c < s.width; c += 64) out[c] = live ? in[c] : 0u;
}

}  // namespace aae
