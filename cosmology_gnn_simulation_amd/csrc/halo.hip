// Backward of the halo exchange: cgnn_halo_return_add.
//
// In the forward a rank sends some of its owned latent rows to the peers that read them as ghosts.  In the backward each
// peer returns the gradient it accumulated on those ghost rows (its sender-CSR sum over its own receivers), and the owner
// adds them into its own gradient rows.  One owned row can be requested by several peers (up to 7 in a 2x2x2 tiling), so
// the add is a short variable-length sum per row: the same atomic-free gather as cgnn_aggregate_csr, with the owner's row
// as the first addend and the result written back in place.  Only the requested rows are touched.
#include "cgnn_common.hpp"

namespace cgnn {

// table[rows[j]] = ((table[rows[j]] + ret[col[p0]]) + ret[col[p0 + 1]]) + ...  for p in [seg_ptr[j], seg_ptr[j + 1]):
// one thread per (row, 16-byte chunk), ascending p.  Four gathers are kept in flight; the adds stay in order.  Rows and
// positions outside the tables are skipped (host logic -- dist.halo_return_plan -- validates the plan; this guard only
// keeps a bad plan from writing outside the tables).
__global__ __launch_bounds__(CGNN_BLOCK) void halo_return_add_kernel(const float* __restrict__ ret, int64_t ret_rows,
                                                                     const int32_t* __restrict__ rows,
                                                                     const int32_t* __restrict__ seg_ptr,
                                                                     const int32_t* __restrict__ col, int64_t n_rows,
                                                                     int chunks, float* __restrict__ table,
                                                                     int64_t table_rows) {
    const int64_t total = n_rows * chunks;
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = w / chunks;
        const int c = (int)(w - j * chunks);
        const int32_t r = rows[j];
        if (r < 0 || r >= table_rows) continue;
        const int p0 = seg_ptr[j], p1 = seg_ptr[j + 1];
        f32x4* dst = reinterpret_cast<f32x4*>(table + ((int64_t)r * chunks + c) * 4);
        f32x4 acc = *dst;
        auto at = [&](int32_t q) -> f32x4 {
            if (q < 0 || q >= ret_rows) return f32x4{0.f, 0.f, 0.f, 0.f};
            return *reinterpret_cast<const f32x4*>(ret + ((int64_t)q * chunks + c) * 4);
        };
        int p = p0;
        for (; p + 3 < p1; p += 4) {
            const f32x4 v0 = at(col[p]), v1 = at(col[p + 1]), v2 = at(col[p + 2]), v3 = at(col[p + 3]);
            acc += v0;
            acc += v1;
            acc += v2;
            acc += v3;
        }
        for (; p < p1; ++p) acc += at(col[p]);
        *dst = acc;
    }
}

}  // namespace cgnn

using namespace cgnn;

extern "C" {

int cgnn_halo_return_add(const float* ret, int64_t num_ret, const int32_t* rows, const int32_t* seg_ptr,
                         const int32_t* col, int64_t num_rows, int32_t width, float* table, int64_t table_rows,
                         void* stream) {
    if (num_rows < 0 || num_ret < 0 || table_rows < 0 || width <= 0 || !seg_ptr ||
        (num_rows > 0 && (!rows || !table || (num_ret > 0 && (!ret || !col))))) {
        set_error("cgnn_halo_return_add: invalid argument");
        return CGNN_ERR_INVALID_ARG;
    }
    if (width % 4 != 0 || width > 256) {
        set_error("cgnn_halo_return_add: width %d is not a multiple of 4 in [4, 256]", width);
        return CGNN_ERR_UNSUPPORTED;
    }
    if (num_rows > table_rows) {
        set_error("cgnn_halo_return_add: %lld rows to add into a table of %lld rows", (long long)num_rows,
                  (long long)table_rows);
        return CGNN_ERR_INVALID_ARG;
    }
    if (num_rows == 0) return CGNN_OK;
    const int chunks = width / 4;
    const int64_t total = num_rows * chunks;
    int64_t blocks = (total + CGNN_BLOCK - 1) / CGNN_BLOCK;
    if (blocks > (1 << 20)) blocks = 1 << 20;
    halo_return_add_kernel<<<(unsigned)blocks, CGNN_BLOCK, 0, (hipStream_t)stream>>>(ret, num_ret, rows, seg_ptr, col,
                                                                                     num_rows, chunks, table, table_rows);
    return check_hip(hipGetLastError(), "cgnn_halo_return_add launch");
}

}  // extern "C"
