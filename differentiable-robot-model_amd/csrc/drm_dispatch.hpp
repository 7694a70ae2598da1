// drm_dispatch.hpp — host side only: what the entry points of the C ABI share when they decide which kernel takes which rows.
// An entry point tries its kernels in the order of the rungs in its own unit: the walk's own code object, the 7-DoF arm kernels, the
// fingers of a hand, an arm that carries a hand, then the loop kernels.  A rung takes the FULL tiles it qualifies for and re-enters
// the entry point for the rest with itself switched off in a copy of the walk.  The per-robot code objects (specialize.py) do NOT
// include this header, so it is not part of their source key.
#pragma once
#include <stdio.h>

#include "drm_common.hpp"

namespace drm {

constexpr int64_t GRID_MAX = 0x7fffffffLL; // a grid dimension is an int
// B has at least one full tile (of `tile` rows) and its full tiles fit an int grid
static inline bool full_tiles_fit(int64_t B, int64_t tile = WAVE) { return B >= tile && B / tile < GRID_MAX; }
// a count of blocks / tiles that is about to become a grid ("batch too large" otherwise)
static inline bool grid_fits(int64_t blocks) { return blocks <= GRID_MAX; }

// all of these pointers are 16-byte aligned (a NULL pointer counts as aligned)
template <class... P>
static inline bool aligned16(const P *...p) { return ((... | (uintptr_t)p) & 15u) == 0; }
// the walk's table can be staged with 16-byte loads
static inline bool table_aligned(const drm_walk *w) { return aligned16(w->ops_f); }

// a serial 7-DoF arm in a table of capacity 8: what the arm kernels (drm_arm_kernels.hip, drm_arm_dynamics.hip) are compiled for
static inline bool arm7_walk(const drm_walk *w) { return (w->shape & DRM_WALK_ARM_CHAIN) && w->capacity == 8 && w->n_dofs == 7; }

// the (K, L) of a DRM_WALK_FINGERS walk the per-finger kernels are compiled for: K = 2 .. 4 serial fingers of L = 2 .. 4 revolute
// joints off the root and nothing else (op k drives DoF k).  The caller tests the DRM_WALK_FINGERS bit itself.
static inline bool fingers_shape(const drm_walk *w, int &K, int &L) {
    K = DRM_WALK_AH_K(w->shape);
    L = DRM_WALK_AH_L(w->shape);
    return K * L == w->n_ops && w->n_dofs == w->n_ops && K >= 2 && K <= 4 && L >= 2 && L <= 4;
}

// the walk for the rows a rung leaves (an odd tile, the ragged tail): without its own kernel of that kind / without that shape bit
static inline drm_walk without_special(const drm_walk &w, int kind) {
    drm_walk rest = w;
    rest.special[kind] = nullptr;
    return rest;
}
static inline drm_walk without_shape(const drm_walk &w, uint32_t bit) {
    drm_walk rest = w;
    rest.shape &= ~bit;
    return rest;
}

static int launch_module_failed(const char *name, hipError_t e) {
    char fmt[96];
    snprintf(fmt, sizeof(fmt), "hipModuleLaunchKernel(%s): %%s", name);
    return fail(DRM_ERR_LAUNCH, fmt, hipGetErrorString(e));
}
// Launches a kernel of a per-robot code object (drm_walk.special[...]) on grid x block threads without dynamic LDS.  The argument
// array is built from references to `args`, in order: their TYPES are the kernel's signature (csrc/drm_static.hpp,
// drm_arm_static.hpp, drm_arm_stream.hpp), so a narrowing such as `int fl = (int)flags` stays explicit at the call site.
template <class... A>
static inline int launch_module(const void *fn, unsigned grid, unsigned block, hipStream_t s, const char *name, A &...args) {
    void *argv[] = {(void *)&args...};
    const hipError_t e = hipModuleLaunchKernel((hipFunction_t)fn, grid, 1, 1, block, 1, 1, 0, s, argv, nullptr);
    return e == hipSuccess ? DRM_OK : launch_module_failed(name, e);
}

} // namespace drm
