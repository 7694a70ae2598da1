// drm_rows.hpp — what the general ("rows") kernels of the tree-sweep entry points share: drm_regressor.hip, drm_lagrangian.hip,
// drm_idd.hip, drm_energy.hip and drm_links.hip, and the record layout of their host loops in drm_cpu.cpp.
//
// A rows kernel walks rows [0, B) in tiles of 64, one lane per row, and between its sweeps a row keeps `state_floats` floats (records
// per op, parked composites per branch point) in the layout [float][64 lanes].  WHERE they live is decided here and nowhere else:
//   * in dynamic LDS where 64 rows of them fit the entry point's limit: one block per tile;
//   * else in the caller's scratch: a persistent grid of at most ROWS_SCRATCH_BLOCKS blocks strides over the tiles, and block b owns
//     floats [b, b + 1) * state_floats * 64 of the scratch for every tile it walks.
// rows_plan() makes the decision, rows_scratch_floats() sizes the scratch from it, rows_launch() launches by it and rows_state() is
// the kernel's side of the same addressing.
//
// Host + device scaffolding of the library's own units: the per-robot code objects (specialize.py) neither include nor need it.
#pragma once
#include <stdint.h>

#include "drm_sample.hpp"
#if defined(__HIPCC__)
#include <initializer_list>

#include "drm_common.hpp"
#include "drm_dispatch.hpp"
#endif

namespace drm {

// Records of N floats each, float i of record k at base[(N k + i) STRIDE].  STRIDE = WAVE with `base` the lane's own first float: the
// [float][64 lanes] layout of the rows kernels.  STRIDE = 1: one row's records in a host array.
template <int N, int STRIDE>
struct Records {
    float *base;
    DRM_HD void put(int k, const float *x) const {
#pragma unroll
        for (int i = 0; i < N; ++i) base[(N * k + i) * STRIDE] = x[i];
    }
    DRM_HD void get(int k, float *x) const {
#pragma unroll
        for (int i = 0; i < N; ++i) x[i] = base[(N * k + i) * STRIDE];
    }
};

#if defined(__HIPCC__)
// ---- device side ----------------------------------------------------------------------
// the control words of a walk for the loop-structured walks (drm_tree.hpp)
struct RowsCtl {
    const int32_t *w0, *w1;
    __device__ RowsCtl(const int32_t *ops_i, int cap) : w0(ops_i + DRM_OPI_W0 * cap), w1(ops_i + DRM_OPI_W1 * cap) {}
    __device__ void raw(int k, int &a, int &b) const { a = w0[k]; b = w1[k]; }
    __device__ int uniform(int r) const { return __builtin_amdgcn_readfirstlane(r); }
};

// the lane's first float of its block's state: dynamic LDS, or the block's slice of the scratch
template <bool IN_LDS>
__device__ __forceinline__ float *rows_state(float *scratch, int state_floats) {
    extern __shared__ __attribute__((aligned(16))) float rows_lds[];
    return (IN_LDS ? rows_lds : scratch + (int64_t)blockIdx.x * state_floats * WAVE) + (threadIdx.x & 63u);
}

// ---- host side ------------------------------------------------------------------------
constexpr int ROWS_SCRATCH_BLOCKS = 2048; // blocks of the persistent grid, each with a slice of the scratch

struct RowsPlan {
    int64_t tiles;          // of 64 rows
    int state_floats;       // per row
    size_t lds;             // dynamic LDS of a block, 0: the state lives in the scratch
    int64_t blocks;         // the grid
    int64_t scratch_floats; // what the caller passes
};
// the general kernel over `rows` rows whose state is `state_floats` floats each, in LDS up to `lds_limit` bytes per block
static inline RowsPlan rows_plan(int64_t rows, int state_floats, int lds_limit) {
    RowsPlan p = {(rows + WAVE - 1) / WAVE, state_floats, sizeof(float) * (size_t)state_floats * WAVE, 0, 0};
    p.blocks = p.tiles;
    if (p.lds <= (size_t)lds_limit) return p;
    p.lds = 0;
    if (p.blocks > ROWS_SCRATCH_BLOCKS) p.blocks = ROWS_SCRATCH_BLOCKS;
    p.scratch_floats = rows > 0 ? p.blocks * state_floats * WAVE : 0;
    return p;
}

// the fused single-tile kernels of these entry points take the full tiles of a 7-DoF arm whose pointers are 16-byte aligned
static inline bool rows_fused(const drm_walk *w, int64_t B, bool aligned) {
    return arm7_walk(w) && aligned && table_aligned(w) && full_tiles_fit(B);
}

// the scratch of a call over B rows of a CHECKED walk: the fused kernel takes B / 64 * 64 rows if the call qualifies and needs none,
// the plan covers the rest
static inline int64_t rows_scratch_floats(const drm_walk *w, int64_t B, bool aligned, int state_floats, int lds_limit) {
    if (B <= 0) return 0;
    const int64_t lo = rows_fused(w, B, aligned) ? B / WAVE * WAVE : 0;
    return rows_plan(B - lo, state_floats, lds_limit).scratch_floats;
}

// zeroes `floats` floats of every output of the list that is not NULL (the rows kernels store structural non-zeros only)
static inline int rows_zero(std::initializer_list<float *> outs, size_t floats, hipStream_t s) {
    for (float *M : outs) {
        if (!M) continue;
        const hipError_t e = hipMemsetAsync(M, 0, sizeof(float) * floats, s);
        if (e != hipSuccess) return fail(DRM_ERR_LAUNCH, "hipMemsetAsync: %s", hipGetErrorString(e));
    }
    return DRM_OK;
}

// Launches the rows kernel by the plan: `in_lds` / `in_scratch` are its <true> / <false> instantiations, `args` its arguments up to
// (scratch, state_floats), which are appended here.  `query` names the entry point's scratch query for the caller who passed none.
template <class KL, class KS, class... A>
static inline int rows_launch(KL in_lds, KS in_scratch, const RowsPlan &p, float *scratch, const char *query, hipStream_t s, A... args) {
    if (p.lds) {
        if (!grid_fits(p.tiles)) return fail(DRM_ERR_UNSUPPORTED, "batch too large");
        hipLaunchKernelGGL(in_lds, dim3((unsigned)p.blocks), dim3(WAVE), p.lds, s, args..., (float *)nullptr, p.state_floats);
    } else {
        if (!scratch) return fail(DRM_ERR_INVALID, "pass %s() floats of scratch", query);
        hipLaunchKernelGGL(in_scratch, dim3((unsigned)p.blocks), dim3(WAVE), 0, s, args..., scratch, p.state_floats);
    }
    return launched();
}
#endif

} // namespace drm
