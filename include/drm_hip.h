/*
 * drm_hip.h — C ABI of the MI355X (gfx950) batched FK / Jacobian / RNEA engine.
 *
 * The reference (facebookresearch/differentiable-robot-model @ v1) has no FFI:
 * its boundary for this path is the Python method surface of
 * `DifferentiableRobotModel` (reference differentiable_robot_model/robot_model.py:87-754).
 * Each entry point below is what a binding for one of those methods calls;
 * the reference interface it replaces is cited per function.  INTEGRATION.md
 * shows the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C, no exceptions cross the boundary; every call returns 0 on
 *     success or a negative DRM_ERR_* code, drm_last_error() (thread-local)
 *     explains it.
 *   - all data pointers are DEVICE pointers to contiguous row-major float32 /
 *     int32 arrays owned by the caller (torch owns them in the Python host);
 *     the library never allocates, frees, copies or synchronises.
 *   - `stream` is a hipStream_t (NULL = the default stream); every call is an
 *     asynchronous launch on that stream and is re-entrant.
 *   - one wavefront (64 lanes) owns a tile of 64 consecutive samples; a lane
 *     owns one sample and walks the robot's flattened tree serially.
 *
 * HOST BUILD.  libdrm_cpu.so (csrc/drm_cpu.cpp) exports the same entry points over HOST pointers for models on
 * device="cpu", the reference's default (robot_model.py:100-104): same arguments, results and error codes; `stream` is
 * ignored and a call returns when its results are written; the forward scratch queries return 0; drm_special_load is
 * DRM_ERR_UNSUPPORTED; drm_fk_mse takes any single-target walk and batch size.  One extra symbol,
 * `drm_cpu_set_threads` (void, takes the thread count as an int).  A host picks the library by where the caller's arrays live — the two never stand
 * in for one another.
 *
 * The robot is handed over as a *walk*: the depth-first list of links a kernel
 * has to visit (flattened on the host once per robot / target set, see
 * differentiable-robot-model_amd/flatten.py) with their constants gathered in
 * walk order, so every per-link constant is a wave-uniform scalar load.
 */
#ifndef DRM_HIP_H
#define DRM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DRM_ABI_VERSION 15

/* ---- layout of one op (= one link) of a walk ---------------------------- */
#define DRM_SPECIAL_KINDS 16 /* drm_walk.special[] (the kinds not named below are reserved and must be NULL): */
#define DRM_SPECIAL_RNEA 0   /*   inverse dynamics          kernel drm_rnea_static  */
#define DRM_SPECIAL_CRBA 1   /*   joint-space inertia matrix   kernel drm_crba_static  */
#define DRM_SPECIAL_FD 2     /*   forward dynamics             kernel drm_fd_static    */
#define DRM_SPECIAL_RNEA_BACKWARD 3 /* reverse-mode inverse dynamics  kernel drm_rnea_backward_static, built with the walk's capacity
                                       as the pitch of its rows of partial sums */
/* ABI 10: serial 7-DoF arms (DRM_WALK_ARM_CHAIN, capacity 8) with the robot's CONSTANTS folded into the instruction stream
 * (csrc/drm_arm_stream.hpp instantiated on a constexpr copy of the walk table: products with exact zeros and ones are gone,
 * no table in LDS).  They cover the 128-row tile pairs of a launch of at least DRM_ARM_STATIC_MIN_PAIRS pairs and ignore
 * ops_f: the host guarantees that the table the handle was built from is the walk's (constant models only). */
#define DRM_SPECIAL_RNEA_ARM 4    /* drm_rnea     kernel "drm_rnea_arm_static", arguments q, qd, qdd, n_pairs, flags, tau              */
#define DRM_SPECIAL_FK_RNEA_ARM 5 /* drm_fk_rnea  kernel "drm_fk_rnea_arm_static", arguments q, qd, qdd, n_pairs, flags, tau, pos, quat;
                                     the SAME handle on the tree walk and on the chain walk it was built for                */
/* ... and the one-sample-per-lane chain walks of the same arm (csrc/drm_arm_static.hpp), one wavefront per 64-row tile: */
#define DRM_SPECIAL_CRBA_ARM 6    /* drm_crba              kernel "drm_crba_arm_static", arguments q, n_tiles, H                       */
#define DRM_SPECIAL_FD_ARM 7      /* drm_forward_dynamics  kernel "drm_fd_arm_static", arguments q, qd, f, n_tiles, flags, qdd          */
#define DRM_SPECIAL_RNEA_BACKWARD_ARM 8 /* drm_rnea_backward with param_mask == 0 (input gradients of a constant model): kernel
                                     "drm_rnea_backward_arm_static", arguments q, qd, qdd, grad_tau, n_tiles, flags, grad_q, grad_qd, grad_qdd */
/* ... and on the 2 .. 4 CHAIN walks of a fan-out FK call (the fingertips of a hand): ONE kernel for all of them, a wavefront per
 * chain, every chain's constants folded in (scalar chain walk, csrc/drm_arm_static.hpp); the SAME handle on every chain walk. */
#define DRM_SPECIAL_FK_FAN_LINKS 9 /* drm_fk_fanout_links  kernel "drm_fk_fan_links_static", arguments q, pos, quat, B (int64)       */
/* ABI 11: NOT a kernel — a device `uint32_t` TICKET word owned by the host, one per walk: zero when a call is enqueued and zero again
 * when it has completed (allocate it zeroed once; calls that use it must not overlap on different streams).  With it the backward
 * entry points that end in a fixed-order reduction of per-wavefront partial sums (drm_fk_mse; drm_fk_backward of a 7-DoF arm
 * chain at a multiple of 64 rows) run as ONE launch: every block publishes its rows and takes a ticket, the block that takes
 * the last one adds the rows — same order, same bits as the separate reduction kernel — and resets the word.  NULL: two
 * launches, as before (the reference's counterpart is autograd's accumulation, robot_model.py:669-713 + examples/
 * learn_kinematics_of_iiwa.py:47-55). */
#define DRM_WALK_TICKET 10
/* ABI 11: a serial 7-DoF arm WITH learnable link parameters (the learn-dynamics workload): drm_rnea_backward's kernel for exactly
 * the set of learnable blocks `drm_walk.reserved0` names (bit k: op k has a learnable parameter; the host built the kernel for
 * that set and for the split into kinematic / dynamic blocks its model has) — the constant blocks of the table are compile-time
 * constants of the kernel, the learnable ones are read from ops_f.  Kernel "drm_rnea_backward_arm_param_static", arguments ops_f,
 * q, qd, qdd, grad_tau, n_tiles, flags, grad_q, grad_qd, grad_qdd, partials; launched with 256-thread blocks, the library's rows of
 * partial sums.  Used when the call's param_mask equals reserved0. */
#define DRM_SPECIAL_RNEA_BACKWARD_ARM_PARAM 11
/* ABI 11: drm_fk_rnea_put's form of DRM_SPECIAL_FK_RNEA_ARM (same code object, same pair of walks): kernel
 * "drm_fk_rnea_arm_put_static", arguments q, qd, qdd, n_pairs, flags, tau, pos, quat and the drm_put struct by value */
#define DRM_SPECIAL_FK_RNEA_ARM_PUT 12
/* ABI 11: DRM_SPECIAL_FD_ARM with TWO samples per lane (csrc/drm_arm_static.hpp forward_dynamics_arm2_static_body): covers the
 * 128-row tile pairs of a launch of at least DRM_ARM_STATIC_MIN_PAIRS pairs; kernel "drm_fd_arm2_static", arguments q, qd, f,
 * n_pairs, flags, qdd */
#define DRM_SPECIAL_FD_ARM2 13
/* ... and DRM_SPECIAL_RNEA_BACKWARD_ARM (input gradients, param_mask == 0) with two samples per lane: kernel
 * "drm_rnea_backward_arm2_static", arguments q, qd, qdd, grad_tau, n_pairs, flags, grad_q, grad_qd, grad_qdd */
#define DRM_SPECIAL_RNEA_BACKWARD_ARM2 14
#define DRM_OPF_STRIDE 32 /* floats per op in ops_f                                            */
/* [0..11] "FT block": R_fixed = Rz(yaw)Ry(pitch)Rx(roll) (rigid_body.py:138-143) and the joint origin xyz
 * ("trans", rigid_body.py:48) interleaved as the 8-byte pairs the packed-FP32 chain kernel multiplies with:
 *   (F00 F01) (F10 F11) (F20 F21) (F02 t0) (F12 t1) (F22 t2)                                          */
#define DRM_OPF_FIJ(i, j) ((j) < 2 ? 2 * (i) + (j) : 6 + 2 * (i)) /* entry (i, j) of R_fixed        */
#define DRM_OPF_TI(i) (7 + 2 * (i))                               /* component i of trans           */
#define DRM_OPF_FT_FLOATS 12
#define DRM_OPF_MASS 12   /* [1] link mass                                                     */
#define DRM_OPF_MCOM 13   /* [3] mass * com                (spatial_vector_algebra.py:323)      */
#define DRM_OPF_IO 16     /* [9] I_c + m S(c)S(c)^T        (spatial_vector_algebra.py:324-327)  */
#define DRM_OPF_DAMP 25   /* [1] joint damping             (robot_model.py:368-373)             */

#define DRM_OPI_STRIDE 10 /* int32 fields per op; ops_i is FIELD-MAJOR: ops_i[field * capacity + k] */
#define DRM_OPI_DOF 0     /* DoF column driven by this link's joint, -1 = fixed joint          */
#define DRM_OPI_PERM 1    /* axis canonicalisation of this link's stored frame, a + 3 * (axis negative):
                             a = 2 joint about local z (or fixed), 0 about local x, 1 about local y
                             (rigid_body.py:149-154).  The constants are pre-multiplied by the signed
                             permutation, the kernels rotate every joint about +z of the stored frame by
                             +q and undo the permutation when a target pose is emitted          */
#define DRM_OPI_CTRL 2    /* the op's control word: every field the kernels branch on, packed so that ONE
                             wide scalar load brings the control flow of the whole walk (a lone wave cannot
                             hide a scalar-load round trip per field and op):
                               bits  0..6  DoF column + 1 (0 = fixed joint)
                               bits  7..9  source + 2     (0 = root, 1 = previous op, 2.. = save slot)
                               bits 10..12 save slot + 1  (0 = none)
                               bits 13..19 output slot + 1 (0 = none)
                               bits 20..22 DRM_OPI_PERM code
                               bit  23     DRM_FLAG_CHILD_IS_NEXT
                               bit  24     identity padding op (kernels may skip it)
                               bit  25     prismatic joint (slides along +z of the stored frame by q)
                               bits 26..31 ordinal of a LEAF op (no child follows it in the walk) among the walk's leaves
                             The unpacked fields below stay in the table for hosts and debuggers       */
#define DRM_OPI_CTRL_PACK(dof, src, save, out, perm, flags)                                                       \
    ((((dof) + 1) & 0x7f) | ((((src) + 2) & 7) << 7) | ((((save) + 1) & 7) << 10) | ((((out) + 1) & 0x7f) << 13) | \
     (((perm) & 7) << 20) | (((flags) & 1) << 23))
#define DRM_OPI_SRC 3     /* parent state: DRM_SRC_PREV, DRM_SRC_ROOT, or a save-slot index    */
#define DRM_OPI_SAVE 4    /* save-slot this op's state is copied to (branch point), -1 = none  */
#define DRM_OPI_OUT 5     /* output slot (target index) this op's pose is written to, -1 = none */
#define DRM_OPI_LINK 6    /* link index in URDF <link> order (informational)                   */
#define DRM_OPI_FLAGS 7   /* DRM_FLAG_*                                                        */

#define DRM_OPI_W0 8      /* the two control words of the loop-structured forward kernels (drm_fk, drm_fk_jacobian,
                             drm_rnea, drm_crba, drm_forward_dynamics of robots that are not 7-DoF arm chains): wider
                             fields than DRM_OPI_CTRL, so walks may have any number of links, 16 save slots and
                             prismatic joints.  W0:
                               bits  0..7  DoF column + 1 (0 = fixed joint)
                               bits  8..15 source + 2     (0 = root, 1 = previous op, 2.. = save slot)
                               bits 16..23 save slot + 1  (0 = none)
                               bit  24     DRM_FLAG_CHILD_IS_NEXT
                               bit  25     identity padding op
                               bit  26     prismatic joint: the link slides along +z of its stored frame by q (URDF
                                           type "prismatic"; everything else that moves is revolute about +z)
                               bits 27..29 DRM_OPI_PERM code                                                    */
#define DRM_OPI_W1 9      /* W1: bits 0..15 output slot + 1 (0 = none), bits 16..31 op index of the parent + 1 (0 = root) */
#define DRM_W0_PACK(dof, src, save, child_next, padding, prismatic, perm)                                       \
    ((((dof) + 1) & 0xff) | ((((src) + 2) & 0xff) << 8) | ((((save) + 1) & 0xff) << 16) | (((child_next) & 1) << 24) | \
     (((padding) & 1) << 25) | (((prismatic) & 1) << 26) | (((perm) & 7) << 27))
#define DRM_W1_PACK(out, parent_op) ((((out) + 1) & 0xffff) | ((((parent_op) + 1) & 0xffff) << 16))

#define DRM_SRC_PREV (-1) /* parent = previous op of the walk                                  */
#define DRM_SRC_ROOT (-2) /* parent = the fixed root link (identity pose, zero velocity)       */
#define DRM_FLAG_CHILD_IS_NEXT 1 /* op k+1 is a child of op k                                  */
#define DRM_MAX_SLOTS 16  /* save slots a walk may use in the forward kernels (kept in LDS)    */
#define DRM_MAX_SLOTS_BACKWARD 6 /* ... and in the backward kernels (what the 3-bit source field of DRM_OPI_CTRL addresses: slots 0 .. 5) */
#define DRM_MAX_OPS 64    /* largest walk the BACKWARD kernels and drm_walk_table take; the forward kernels are bounded
                             by the LDS their per-link records need (DRM_ERR_UNSUPPORTED beyond that, ~70 links) */
#define DRM_MAX_SEGMENTS 8 /* independent sub-walks (sub-trees hanging off the fixed root) a dynamics launch fans out
                              over the wavefronts of a block                                      */
#define DRM_MAX_DOFS 64   /* largest supported number of DoF columns                           */

/* drm_walk.shape */
#define DRM_WALK_ARM_CHAIN 1 /* a serial chain: ops 0..n_dofs-1 are moving joints driving DoF columns
                                0..n_dofs-1 in order, every later op is a fixed joint or padding  */
#define DRM_WALK_SERIAL_CHAIN 2 /* a serial chain of ANY shape: op 0 hangs off the root, every other op off the previous one,
                                no save slots, the single target is the last op; revolute, prismatic and fixed ops
                                in any order, any DoF columns.  Walks of capacity 4 / 8 / 12 / 16 with this bit take the
                                straight-line chain kernels (drm_chain_kernels.hip) in drm_fk / drm_fk_jacobian / drm_fk_fanout */
#define DRM_WALK_ARM_HAND 4 /* "an arm that carries a hand": ops 0 .. P-1 form a serial chain (op 0 off the root) and the remaining
                              K * L ops are K serial sub-chains of L ops each, every one hanging off op P-1, in walk order.
                              P, K, L travel in the top byte of shape: */
#define DRM_WALK_AH_P(shape) ((int)(((uint32_t)(shape) >> 24) & 0xf))
#define DRM_WALK_AH_K(shape) ((int)(((uint32_t)(shape) >> 28) & 0x3) + 1)
#define DRM_WALK_AH_L(shape) ((int)(((uint32_t)(shape) >> 30) & 0x3) + 1)
#define DRM_WALK_AH_PACK(P, K, L) ((uint32_t)DRM_WALK_ARM_HAND | ((uint32_t)(P) << 24) | ((uint32_t)((K) - 1) << 28) | ((uint32_t)((L) - 1) << 30))
#define DRM_WALK_FINGERS 16 /* K serial chains of L revolute ops each, every chain hanging off the root, op k driving DoF column k
                              (the fingers of a hand once the fixed joints are folded: Allegro 4 x 4, TriFinger 3 x 3); K and L in
                              the top byte as for DRM_WALK_ARM_HAND (DRM_WALK_AH_K / DRM_WALK_AH_L; P = 0) */
#define DRM_WALK_NO_PRISMATIC 32 /* no op of the walk is a prismatic joint (the two-samples-per-lane fan-out FK kernel asks for it) */
#define DRM_WALK_CHAIN_DOFS 128 /* chain_dof1 / chain_prismatic below are filled (serial chains of <= 16 ops): the straight-line
                                  chain kernels take the DoF columns from the launch arguments instead of reading the control words
                                  first — one dependent memory round trip less before a wavefront's joint angles are requested */
#define DRM_WALK_FK_FAN 64 /* a many-target FK walk (DRM_WALK_TARGETS_ORDERED) that splits behind a hub: ops [0, prefix_end) are
                              what every sub-tree hangs off, seg_begin[j] .. seg_begin[j + 1] the ops of wavefront j's sub-trees (the
                              first op of every range but the first reads its parent's pose from a save slot or the root) */
#define DRM_WALK_TARGETS_ORDERED 8 /* the ops with an output slot carry slots 0, 1, 2, ... in walk order: drm_fk with more than
                                  eight targets then writes its outputs a group of eight consecutive slots at a time */
#define DRM_WALK_LEAVES(shape) (((shape) >> 16) & 0xff) /* number of leaf ops (ops no child follows), see DRM_OPI_CTRL */
#define DRM_WALK_BRANCH_DEPTH(shape) (((shape) >> 8) & 0xff) /* 1 + the largest op index that is a branch
                                point (0: none): sizes the per-ancestor slot records of drm_crba /
                                drm_forward_dynamics                                               */

/* flags of drm_rnea */
#define DRM_RNEA_GRAVITY 1 /* base acceleration (0,0,+9.81)   (robot_model.py:344-350)         */
#define DRM_RNEA_DAMPING 2 /* tau += damping * qd             (robot_model.py:368-373)         */
/* flags of drm_forward_dynamics_rollout (ABI 14), beside DRM_RNEA_GRAVITY / DRM_RNEA_DAMPING */
#define DRM_ROLLOUT_EXPLICIT_EULER 4 /* q += dt * qd_t, then qd += dt * qdd_t (default: semi-implicit Euler) */
/* flags of drm_inverse_kinematics (ABI 15) */
#define DRM_IK_POSITION_ONLY 1 /* target_pos only: a 3 x 3 system, rot_err written as 0 */
#define DRM_IK_COMPOSED 2      /* force the composed path on every row (tests, A/B) */
/* flags of drm_operational_space, beside DRM_RNEA_GRAVITY / DRM_RNEA_DAMPING */
#define DRM_OSC_POSITION_ONLY 8 /* J = lin_jac alone: a 3 x 3 task space */
#define DRM_OSC_COMPOSED 16     /* force the composed path on every row (tests, A/B) */
/* flag of drm_forward_dynamics_derivatives, beside DRM_RNEA_GRAVITY / DRM_RNEA_DAMPING */
#define DRM_FDD_COMPOSED 32     /* force the composed path on every row (tests, A/B) */
/* flags of drm_rnea_regressor, beside DRM_RNEA_GRAVITY / DRM_RNEA_DAMPING */
#define DRM_REGRESSOR_COMPOSED 64  /* force the general kernel on every row (tests, A/B) */
/* flag of drm_lagrangian_dynamics */
#define DRM_LAGRANGIAN_COMPOSED 128 /* force the general kernel on every row (tests, A/B) */
/* flag of drm_rnea_derivatives, beside DRM_RNEA_GRAVITY / DRM_RNEA_DAMPING */
#define DRM_IDD_COMPOSED 256        /* force the general kernel on every row (tests, A/B) */
/* flag of drm_energy */
#define DRM_ENERGY_COMPOSED 512     /* force the general kernel on every row (tests, A/B) */

/* error codes */
#define DRM_OK 0
#define DRM_ERR_INVALID (-1)     /* bad argument (NULL pointer, negative size, capacity ...)   */
#define DRM_ERR_UNSUPPORTED (-2) /* walk larger than any compiled kernel                       */
#define DRM_ERR_LAUNCH (-3)      /* HIP reported a launch error                                */

/*
 * A walk, as produced by flatten.build_walk().  ops_f / ops_i hold `capacity`
 * rows: n_ops real ones followed by identity padding (fixed joint, F = I,
 * t = 0, mass 0, DRM_SRC_PREV); capacity is 4 or 8 for walks of up to 8 links (the
 * 7-DoF arm kernels are compiled for 8 and run the walk as straight-line code), n_ops rounded up to a
 * multiple of 4 beyond that (every other kernel loops over the n_ops links).
 */
typedef struct drm_walk {
    const float *ops_f;   /* device [capacity, DRM_OPF_STRIDE]                               */
    const int32_t *ops_i; /* device [DRM_OPI_STRIDE, capacity]  (field-major)                */
    int32_t n_ops;        /* links visited                                                   */
    int32_t capacity;     /* rows of ops_f / ops_i (>= n_ops, a multiple of 4)               */
    int32_t n_dofs;       /* n = row width of q / qd / qdd / tau and Jacobian column count   */
    int32_t n_slots;      /* save slots used (<= DRM_MAX_SLOTS; backward kernels: <= DRM_MAX_SLOTS_BACKWARD) */
    uint64_t dof_mask;    /* bit d set <=> DoF d is driven by an op of this walk             */
    int32_t target_perm;  /* drm_fk_jacobian: DRM_OPI_PERM code (0..5) of the target (last real) op */
    int32_t shape;        /* DRM_WALK_* bits describing the walk, so launchers can pick a specialised kernel */
    /* Segments: sub-trees that hang off the fixed root are independent dynamics problems (the fingers of a hand on a
     * fixed palm).  Ops seg_begin[s] .. seg_begin[s+1]-1 form segment s (a run of whole root-level sub-trees, in walk
     * order); its joints drive the DoF columns seg_dof_lo[s] .. seg_dof_lo[s] + seg_dof_cnt[s] - 1 and no others.
     * A block of n_segments wavefronts owns 64 samples, wavefront s walks segment s.  n_segments = 1: the whole walk. */
    int32_t n_segments;
    int32_t seg_begin[DRM_MAX_SEGMENTS + 1];
    int32_t seg_dof_lo[DRM_MAX_SEGMENTS];
    int32_t seg_dof_cnt[DRM_MAX_SEGMENTS];
    int32_t prefix_end;   /* ops 0 .. prefix_end-1 are STATIC (fixed joints hanging off the root: a mounting plate, the base
                             link of a TriFinger); every segment replays them before its own ops, forward sweeps only */
    int32_t seg_leaf_begin[DRM_MAX_SEGMENTS + 1]; /* leaf ordinals (DRM_OPI_CTRL bits 26..31) of segment s:
                             seg_leaf_begin[s] .. seg_leaf_begin[s+1]-1 (leaves are numbered in walk order, those of the
                             prefix first); read by the RNEA backward kernel when it fans the segments out over wavefronts */
    uint8_t chain_dof1[16];   /* DRM_WALK_CHAIN_DOFS: 1 + the DoF column op k reads, 0 for an op that does not move (fixed joint,
                                 padding) — what DRM_OPI_W0 says, for the first 16 ops of a serial chain */
    uint32_t chain_prismatic; /* DRM_WALK_CHAIN_DOFS: bit k set <=> op k slides */
    uint32_t reserved0;       /* ABI 11: the param_mask special[DRM_SPECIAL_RNEA_BACKWARD_ARM_PARAM] was built for (else 0) */
    /* ABI 9: per-robot STRAIGHT-LINE kernels for THIS walk (a whole-tree dynamics walk of any shape), or NULL.  Handles from
     * drm_special_load() of a code object the host built from csrc/drm_static.hpp instantiated on this walk's tree
     * (differentiable-robot-model_amd/specialize.py writes and compiles it: ~2 s with hipcc, cached).  When set, the full
     * 64-row tiles of drm_rnea / drm_crba / drm_forward_dynamics run it instead of the loop kernels (no scratch; drm_rnea at any pointer alignment); a ragged tail and every
     * walk without a handle behave as before.  The host guarantees that a handle was built for exactly this walk (n_ops,
     * parents, DoF columns, joint kinds).
     * ABI 10: 12 slots.  Kinds 4 .. 9 (DRM_SPECIAL_*_ARM, DRM_SPECIAL_FK_FAN_LINKS above) — and kinds 0 .. 3 when the host built
     * them with the table as compile-time constants — carry the walk's CONSTANTS in their instruction stream and do not read
     * ops_f: the host attaches them to constant models only and guarantees that the table they were built from is this walk's. */
    const void *special[DRM_SPECIAL_KINDS];
} drm_walk;

int drm_abi_version(void);
/* Load a code object (what `hipcc --genco --offload-arch=gfx950` writes) and look up one kernel: the handle for
 * drm_walk.special[].  The module stays loaded for the life of the process. */
int drm_special_load(const char *code_object_path, const char *kernel_name, const void **function_out);
int drm_walk_sizeof(void); /* sizeof(struct drm_walk) as the library was compiled: a binding checks its mirror of the struct against it */
const char *drm_last_error(void);

/*
 * Forward kinematics of T target links.
 * Replaces DifferentiableRobotModel.compute_forward_kinematics (robot_model.py:223-248:
 * update_kinematic_state 139-195 + CoordinateTransform.get_quaternion
 * spatial_vector_algebra.py:108-136) and, with T = all links,
 * compute_forward_kinematics_all_links (robot_model.py:197-221).
 *   q    [B, n]      joint angles
 *   pos  [B, T, 3]   world position of each target link frame
 *   quat [B, T, 4]   world orientation, xyzw
 * Target t is the op whose DRM_OPI_OUT == t.
 */
int drm_fk(const drm_walk *walk, const float *q, int64_t B, int32_t n_targets,
           float *pos, float *quat, void *stream);

/*
 * Forward kinematics of T target links with LINK-MAJOR outputs: every link's poses a contiguous array.
 * Replaces DifferentiableRobotModel.compute_forward_kinematics_all_links (robot_model.py:197-221), which hands out one
 * (pos [B, 3], quat [B, 4]) pair per link name.
 *   q    [B, n]
 *   pos  [T, B, 3]   link t's positions are pos + t * B * 3
 *   quat [T, B, 4]   xyzw
 * Target t is the op whose DRM_OPI_OUT == t (any order).  A walk with DRM_WALK_FK_FAN is fanned out over wavefronts.
 */
int drm_fk_links(const drm_walk *walk, const float *q, int64_t B, int32_t n_targets, float *pos, float *quat, void *stream);

/*
 * drm_fk for 2 .. 4 targets whose root->target chains are (nearly) disjoint — the fingertips of a hand: `chains[t]`
 * is the single-target walk of target t (all with the same capacity and n_dofs, no branch points); a block of T
 * wavefronts owns 64 samples and wavefront t walks only chain t (the "per-link fan-out" of the parent-index tree).
 * Same outputs as drm_fk with the merged walk: pos [B, T, 3], quat [B, T, 4].
 */
int drm_fk_fanout(const drm_walk *chains, int32_t n_chains, const float *q, int64_t B, float *pos, float *quat,
                  void *stream);

/* The same with LINK-MAJOR outputs, pos [T, B, 3] / quat [T, B, 4] (chain t's poses a contiguous array, as drm_fk_links): each
 * wavefront writes its own chain's arrays, the block shares no tile.  What a caller of compute_forward_kinematics for several
 * fingertips wants: T (pos [B, 3], quat [B, 4]) pairs (robot_model.py:223-248 called once per link). */
int drm_fk_fanout_links(const drm_walk *chains, int32_t n_chains, const float *q, int64_t B, float *pos, float *quat,
                        void *stream);

/*
 * FK + geometric Jacobian of ONE target link; the walk is the root->link chain
 * and its last op is the target.
 * Replaces DifferentiableRobotModel.compute_endeffector_jacobian (robot_model.py:626-667),
 * which itself runs compute_forward_kinematics first (robot_model.py:641).
 *   pos [B,3], quat [B,4] (either may be NULL), lin_jac / ang_jac [B, 3, n];
 *   columns of DoFs that are not on the chain are written as zeros.
 */
int drm_fk_jacobian(const drm_walk *walk, const float *q, int64_t B,
                    float *pos, float *quat, float *lin_jac, float *ang_jac, void *stream);

/*
 * Recursive Newton-Euler inverse dynamics over the whole tree.
 * Replaces DifferentiableRobotModel.compute_inverse_dynamics (robot_model.py:305-375:
 * update_kinematic_state + update_joint_acc rigid_body.py:159-165 +
 * iterative_newton_euler robot_model.py:250-303).  With qdd = NULL the joint
 * accelerations are zero: compute_non_linear_effects (robot_model.py:377-400).
 *   q, qd, qdd [B, n]  ->  tau [B, n];  flags = DRM_RNEA_GRAVITY | DRM_RNEA_DAMPING
 *   scratch   drm_rnea_scratch_floats(walk, B) floats owned by the caller: robots with a long segment (an arm carrying a
 *             gripper or a hand) keep the body force of every link there between the two sweeps,
 *             [resident block][link][6][64] — bounded by what the device holds at once, not by B.  0 for 7-DoF arms and
 *             for hands (short independent fingers): scratch is then never touched and may be NULL
 */
int64_t drm_rnea_scratch_floats(const drm_walk *walk, int64_t B);
int64_t drm_rnea_scratch_floats_aligned(const drm_walk *walk, int64_t B); /* the caller guarantees 16-byte aligned pointers (see Alignment) */
int drm_rnea(const drm_walk *walk, const float *q, const float *qd, const float *qdd, int64_t B,
             int32_t flags, float *tau, float *scratch, void *stream);

/*
 * Inverse dynamics AND the pose of one link in one call: what a caller of the reference gets from
 * compute_inverse_dynamics (robot_model.py:305-375) followed by compute_forward_kinematics (robot_model.py:223-248) on
 * the same q — the reference walks the tree twice, re-evaluating every joint transform (BASELINE configuration 3).
 *   tree      the whole-tree walk drm_rnea takes;   chain   the root->link walk drm_fk takes (one target)
 *   target_op index of the FK target among the ops of `tree`, or -1 if unknown: when the tree is a serial 7-DoF arm and
 *             the target is its last link, both results come from ONE fused launch (one read of q, one sin/cos
 *             evaluation, one constant table); otherwise the two walks are launched one after the other.
 *             FOLDED TREES: a host may leave links behind fixed leaf joints (an end-effector frame) out of `tree` after
 *             adding their inertia to their parents' rows (the dynamics are unchanged; fewer ops).  If `tree` then holds
 *             exactly the n moving joints of a serial 7-DoF arm and `chain` is that arm up to the target, the fused launch
 *             reads ONE table, chain->ops_f: the caller guarantees that its first n rows carry the same constants as
 *             tree->ops_f (both gathered from the same folded link table); target_op is ignored (-1).
 *   q, qd, qdd [B, n] (qdd may be NULL)  ->  tau [B, n], pos [B, 3], quat [B, 4];  flags as for drm_rnea.
 *   scratch   drm_rnea_scratch_floats(tree, B) floats, as for drm_rnea (0 for the fused launch)
 * Results are bit-identical to drm_rnea + drm_fk.
 */
int drm_fk_rnea(const drm_walk *tree, const drm_walk *chain, int32_t target_op, const float *q, const float *qd,
                const float *qdd, int64_t B, int32_t flags, float *tau, float *pos, float *quat, float *scratch, void *stream);

/*
 * ABI 11: drm_fk_rnea with a ONE-SIDED GATHER of its outputs — the exchange step of a batch sharded over the GPUs of a node
 * (BASELINE configuration 3; SURVEY.md §8e asked for direct peer writes instead of a collective after the kernel).  Besides its own
 * tau / pos / quat the call writes the same rows into up to DRM_MAX_PEERS destination sets at row `row_offset`: the gathered arrays
 * of the peers (their device memory, mapped into this process once by hipIpcOpenMemHandle — differentiable-robot-model_amd/
 * distributed.py PeerGather does the exchange), or of rank 0 only.  For a serial 7-DoF arm with its own fused kernel attached
 * (drm_walk.special[DRM_SPECIAL_FK_RNEA_ARM_PUT]) the kernel's epilogue stores every tile to all destinations as it leaves the
 * wavefront — the xGMI links are busy while the walk runs, no collective launch, no second pass over the data; every other walk,
 * and ragged tails, are computed by drm_fk_rnea and copied (hipMemcpyAsync on `stream`, one copy per destination and array).
 * A destination pointer may be NULL (that array is not wanted there, e.g. torques only).  Completion: stream order on THIS GPU —
 * a consumer on another GPU needs its own synchronisation with this rank (a barrier, a flag), as after any one-sided put.
 * The reference has no counterpart (one process, one device: robot_model.py:87-137); the rows are bit-identical to drm_fk_rnea's.
 */
#define DRM_MAX_PEERS 8
typedef struct drm_put {
    int32_t n_peers;             /* 0 .. DRM_MAX_PEERS destination sets                                              */
    int32_t reserved;
    int64_t row_offset;          /* this call's first row in the destinations' arrays (a multiple of 4 for the in-kernel form) */
    float *tau[DRM_MAX_PEERS];   /* [>= row_offset + B, n] each, or NULL                                              */
    float *pos[DRM_MAX_PEERS];   /* [>= row_offset + B, 3]                                                            */
    float *quat[DRM_MAX_PEERS];  /* [>= row_offset + B, 4]                                                            */
} drm_put;
int drm_fk_rnea_put(const drm_walk *tree, const drm_walk *chain, int32_t target_op, const float *q, const float *qd, const float *qdd,
                    int64_t B, int32_t flags, float *tau, float *pos, float *quat, float *scratch, const drm_put *put, void *stream);

/*
 * Joint-space inertia matrix over the whole tree (composite-rigid-body algorithm).
 * Replaces DifferentiableRobotModel.compute_lagrangian_inertia_matrix (robot_model.py:402-450: n + 1
 * compute_inverse_dynamics passes, column j = ID(q, 0, e_j) - ID(q, 0, 0)).  The gravity / damping flags of the
 * reference cancel out of that difference, so there are none here.
 *   q [B, n]  ->  H [B, n, n]   (symmetric; entries of joints on different branches are zero)
 *   scratch   drm_crba_scratch_floats(walk, B) floats owned by the caller: robots with a long segment (an arm carrying a
 *             gripper or a hand) collect the lower triangle of H there, [resident block][segment][entry][64] — bounded by
 *             what the device holds at once, not by B — before its rows are written.  0 for 7-DoF arms and for hands
 *             (short independent fingers): scratch is then never touched and may be NULL
 */
int64_t drm_crba_scratch_floats(const drm_walk *walk, int64_t B);
int64_t drm_crba_scratch_floats_aligned(const drm_walk *walk, int64_t B); /* the caller guarantees 16-byte aligned pointers (see Alignment) */
int drm_crba(const drm_walk *walk, const float *q, int64_t B, float *H, float *scratch, void *stream);

/*
 * Forward dynamics over the whole tree: joint accelerations produced by joint torques f in state (q, qd).
 * Replaces DifferentiableRobotModel.compute_forward_dynamics (robot_model.py:487-624, articulated-body
 * algorithm).  flags as for drm_rnea: DRM_RNEA_GRAVITY = base acceleration (0,0,+9.81) (robot_model.py:527-533),
 * DRM_RNEA_DAMPING = the damping torques damping * qd are taken off f first (robot_model.py:515-521; the
 * caller's f is NOT modified, unlike the reference, which subtracts in place).
 *   q, qd, f [B, n]  ->  qdd [B, n]
 * Three kernels: 7-DoF arm chains and robots whose segments are all short (the fingers of a hand) form H and the bias
 * torques and solve H qdd = f - nle by an L^T D L factorisation in registers / LDS (the same elimination, H is at most
 * 7 x 7 there); every other robot (an arm carrying a gripper or a hand, a mobile manipulator) runs the articulated-body
 * recursion itself, three sweeps over the walk with 8 floats per link and sample between them.
 *   scratch   drm_forward_dynamics_scratch_floats(walk, B) floats owned by the caller: the per-link records of the
 *             articulated-body sweeps, [resident block][link][8][64] — bounded by what the device holds at once (tens of
 *             MB), not by B.  0 for the arm and finger kernels: scratch is then never touched and may be NULL
 */
int64_t drm_forward_dynamics_scratch_floats(const drm_walk *walk, int64_t B);
int64_t drm_forward_dynamics_scratch_floats_aligned(const drm_walk *walk, int64_t B); /* the caller guarantees 16-byte aligned pointers (see Alignment) */
int drm_forward_dynamics(const drm_walk *walk, const float *q, const float *qd, const float *f, int64_t B,
                         int32_t flags, float *qdd, float *scratch, void *stream);

/*
 * ABI 14: T steps of forward dynamics and an Euler integrator in one call (sampling-based MPC, fitting dynamics to trajectories,
 * trajectory optimisation through the dynamics).  Step t = 0 .. T-1 computes qdd_t = drm_forward_dynamics(q_t, qd_t, tau_t)
 * with the same flags, then
 *   semi-implicit Euler (default):             qd_{t+1} = qd_t + dt * qdd_t,  q_{t+1} = q_t + dt * qd_{t+1}
 *   DRM_ROLLOUT_EXPLICIT_EULER:                q_{t+1} = q_t + dt * qd_t,     qd_{t+1} = qd_t + dt * qdd_t
 * (each update one fused multiply-add).  All arrays are TIME-MAJOR: step t's slab is a contiguous [B, n] array.
 *   q0, qd0 [B, n], tau [T, B, n]  ->  q_traj, qd_traj [T, B, n]: the states after steps 1 .. T;
 *   qdd_traj [T, B, n]: qdd_t, or NULL (the backward pass needs it).  tau is not modified.
 * Full 64-row tiles of 7-DoF arm chains and of hands (DRM_WALK_FINGERS) run ONE kernel that keeps the state in registers across
 * the T steps (84 B per row and step: tau in, q and qd out; 112 B with qdd_traj); every other robot, the ragged tail of a launch
 * and misaligned pointers run drm_forward_dynamics on each step's slab followed by a small element-wise integrator kernel.
 *   scratch   drm_forward_dynamics_rollout_scratch_floats(walk, B) floats: qdd of the composed steps when qdd_traj is NULL, and
 *             what drm_forward_dynamics asks for; 0 when the fused kernel covers every row (scratch may then be NULL)
 * DRM_ERR_INVALID for T < 1 or a dt that is not finite and positive; B == 0 returns DRM_OK.  Asynchronous on `stream`.
 */
int64_t drm_forward_dynamics_rollout_scratch_floats(const drm_walk *walk, int64_t B);
int64_t drm_forward_dynamics_rollout_scratch_floats_aligned(const drm_walk *walk, int64_t B); /* 16-byte aligned pointers (see Alignment) */
int drm_forward_dynamics_rollout(const drm_walk *walk, const float *q0, const float *qd0, const float *tau, int64_t B, int32_t T,
                                 float dt, int32_t flags, float *q_traj, float *qd_traj, float *qdd_traj, float *scratch,
                                 void *stream);

/*
 * ABI 15: batched inverse kinematics of one link by damped least squares, up to max_iters updates per row in one call.
 * Row b starts at q0[b] and iteration i = 0, 1, .., max_iters evaluates at q_i:
 *   p, c, Jp, Jw   = drm_fk_jacobian(q_i) of the walk's target (c an xyzw quaternion)
 *   e_p = target_pos - p;  e_q = t (x) conj(c) with t = target_quat normalised (Hamilton product, negated if its w < 0);
 *   with v = e_q.xyz, s = |v|, theta = 2 atan2(s, e_q.w):  e_R = v theta / s  (2 v when s == 0)
 *   pos_err = |e_p|, rot_err = theta in [0, pi]
 *   converged iff pos_err <= tol_pos && rot_err <= tol_rot.  A converged row, or every row at i == max_iters, writes q_i,
 *   err = (pos_err, rot_err) and iters = i, and stops.  Otherwise, with J = [Jp; Jw] (6 x n) and e = [e_p; e_R]:
 *   q_{i+1} = min(max(q_i + step * J^T (J J^T + damping^2 I)^-1 e, lower), upper)   (Cholesky, fp32)
 * DRM_IK_POSITION_ONLY: J = Jp, e = e_p (3 x 3), convergence on pos_err alone, rot_err = 0; target_quat must be NULL then,
 * and only then.  A row whose inputs are not finite never converges and returns non-finite values; it changes no other row.
 *   q0 [B, n], target_pos [B, 3], target_quat [B, 4] or NULL  ->  q [B, n], err [B, 2], iters [B] (may be NULL)
 *   lower, upper  [n] device arrays, both or neither (NULL: no clamp); +-inf entries leave a DoF free
 * Full 64-row tiles of 7-DoF arm chains (DRM_WALK_ARM_CHAIN, capacity 8, target_perm 2, 16-byte aligned pointers) run ONE kernel
 * that keeps q, the target and the Jacobian in registers across the iterations and leaves the loop when every row of the
 * wavefront has stopped.  Every other robot, the ragged tail, misaligned pointers and DRM_IK_COMPOSED run max_iters + 1 rounds
 * of drm_fk_jacobian into the scratch followed by a one-lane-per-row update kernel, without a host synchronisation.
 *   scratch   drm_inverse_kinematics_scratch_floats_aligned(walk, B) floats when every pointer is 16-byte aligned (0 when the
 *             fused kernel covers every row; scratch may then be NULL), drm_inverse_kinematics_scratch_floats(walk, B) floats
 *             otherwise and with DRM_IK_COMPOSED (the composed path's FK + Jacobian, its input and a flag of every row)
 * DRM_ERR_INVALID for bad arguments (max_iters < 0, damping or step not finite and > 0, a tolerance not finite and >= 0);
 * B == 0 returns DRM_OK.  Asynchronous on `stream`.
 */
int64_t drm_inverse_kinematics_scratch_floats(const drm_walk *walk, int64_t B);
int64_t drm_inverse_kinematics_scratch_floats_aligned(const drm_walk *walk, int64_t B); /* 16-byte aligned pointers (see Alignment) */
int drm_inverse_kinematics(const drm_walk *walk, const float *q0, const float *target_pos, const float *target_quat, int64_t B,
                           int32_t max_iters, float damping, float step, float tol_pos, float tol_rot, const float *lower,
                           const float *upper, int32_t flags, float *q, float *err, int32_t *iters, float *scratch, void *stream);

/*
 * Operational-space dynamics of one link in one call (additive to ABI 15): what a task-space controller needs every tick, and
 * what a caller otherwise composes from drm_fk_jacobian, drm_crba, drm_rnea with qdd = NULL and a chain of small dense solves.
 * With H(q) qdd + nle(q, qd) = tau (nle as drm_rnea with qdd = NULL and the same gravity / damping flags), J = [lin_jac; ang_jac]
 * of drm_fk_jacobian (m = 6 rows; m = 3, lin_jac alone, with DRM_OSC_POSITION_ONLY) and A = J H^-1 J^T + reg^2 I (m x m):
 *   inertia    [B, m, m]  A^-1, the task-space inertia (symmetric)
 *   jbar       [B, n, m]  H^-1 J^T inertia, the dynamically consistent inverse of J
 *   bias_acc   [B, m]     Jdot qd: the world-frame classical acceleration of the link origin (rows 0-2) and the angular
 *                         acceleration of the link (rows 3-5) at zero joint accelerations, gravity absent
 *   bias_force [B, m]     inertia (J H^-1 nle - Jdot qd)
 * so that tau = J^T (inertia a + bias_force) produces the link acceleration a when reg = 0.
 *   tree, chain  as for drm_fk_rnea: the whole-tree walk and the root->link walk, folded trees allowed in the same way
 *   q, qd [B, n];  flags: DRM_RNEA_GRAVITY | DRM_RNEA_DAMPING | DRM_OSC_POSITION_ONLY | DRM_OSC_COMPOSED;  reg >= 0
 *   Any of the four outputs may be NULL: that array is not written.  qd may be NULL when neither bias_acc nor bias_force is asked for.
 * A serial 7-DoF arm whose target is the chain's last link (where drm_fk_rnea fuses), full 64-row tiles, 16-byte aligned pointers:
 * ONE kernel, one wavefront per tile — one sin / cos evaluation shared by the bias torques, H and the Jacobian, H factorised once
 * (L^T D L) in registers and solved against the m rows of J, A inverted by Cholesky, no intermediate in HBM (56 B in per row).
 * Every other robot, a mid-chain target, the ragged tail, misaligned pointers and DRM_OSC_COMPOSED: drm_fk_jacobian, drm_crba and
 * drm_rnea into the scratch, then a finish kernel with one lane per row.  A row whose q or qd is not finite gets non-finite
 * outputs and changes no other row; a singular configuration with reg = 0 gives a huge or non-finite inertia on that row only.
 *   scratch   drm_operational_space_scratch_floats_aligned floats when every pointer (scratch included) is 16-byte aligned (0 when
 *             the fused kernel covers every row; scratch may then be NULL), drm_operational_space_scratch_floats floats otherwise
 *             and with DRM_OSC_COMPOSED
 * DRM_ERR_INVALID when reg is negative or not finite, a required pointer is NULL or every output is NULL; B == 0 returns DRM_OK.
 * Asynchronous on `stream`, never a host synchronisation.
 */
int64_t drm_operational_space_scratch_floats(const drm_walk *tree, const drm_walk *chain, int64_t B);
int64_t drm_operational_space_scratch_floats_aligned(const drm_walk *tree, const drm_walk *chain, int64_t B);
int drm_operational_space(const drm_walk *tree, const drm_walk *chain, const float *q, const float *qd, int64_t B, int32_t flags,
                          float reg, float *inertia, float *jbar, float *bias_acc, float *bias_force, float *scratch, void *stream);

/*
 * The linearisation of forward dynamics about a state in one call (additive to ABI 15): what iLQR / DDP, LQR, linearised MPC and an
 * EKF need at every knot, and what a caller otherwise gets from n backward passes through drm_forward_dynamics with one-hot
 * cotangents.  With ID(q, qd, qdd) = H(q) qdd + nle(q, qd) (drm_rnea with the same gravity / damping flags) and qdd = H^-1 (f - nle):
 *   qdd   [B, n]      what drm_forward_dynamics computes from the same inputs
 *   dq    [B, n, n]   [b, i, j] = d qdd_i / d q_j  = -(H^-1 dID/dq)[i, j] at (q, qd, qdd)
 *   dqd   [B, n, n]   [b, i, j] = d qdd_i / d qd_j = -(H^-1 dID/dqd)[i, j]; with DRM_RNEA_DAMPING it includes -H^-1 diag(damping)
 *   minv  [B, n, n]   H(q)^-1 = d qdd / d f, symmetric to the bit
 *   q, qd, f [B, n] (f is not modified);  flags: DRM_RNEA_GRAVITY | DRM_RNEA_DAMPING | DRM_FDD_COMPOSED.  No output may be NULL.
 * Row k of dID/dq and dID/dqd is the reverse sweep of RNEA seeded with grad_tau = e_k; the outputs are 3 n solves with ONE L^T D L
 * factorisation of H.  Serial 7-DoF arm chains, full 64-row tiles, 16-byte aligned pointers (what drm_forward_dynamics' arm kernel
 * takes): ONE kernel, one wavefront per tile, one row per lane — one sin / cos evaluation, H by the composite walk factorised once
 * in registers, qdd, H^-1, then the n sweeps and the 2 n solves; the three matrices leave through LDS in 16-byte stores (84 B in,
 * 616 B out per row, nothing else through HBM).  A walk that carries its robot's own forward-dynamics kernel (special[DRM_SPECIAL_FD*])
 * gets qdd from drm_forward_dynamics in a second launch: the same values as that call, to the bit.  Every other robot, the ragged tail, misaligned pointers and DRM_FDD_COMPOSED:
 * drm_forward_dynamics, drm_crba and n calls of drm_rnea_backward (grad_tau = e_k) into the scratch, then a finish kernel with one
 * lane per row that factorises H, inverts and solves (n <= 16: in registers; else in LDS, or in the scratch where 64 rows do not
 * fit).  A row whose q, qd or f is not finite gets non-finite outputs and changes no other row.
 *   scratch   drm_forward_dynamics_derivatives_scratch_floats_aligned floats when every pointer (scratch included) is 16-byte
 *             aligned (0 when the fused kernel covers every row; scratch may then be NULL),
 *             drm_forward_dynamics_derivatives_scratch_floats floats otherwise and with DRM_FDD_COMPOSED
 * DRM_ERR_UNSUPPORTED for a walk the backward kernels do not take (more than DRM_MAX_OPS ops or DRM_MAX_SLOTS_BACKWARD save slots);
 * DRM_ERR_INVALID when a pointer is NULL; B == 0 returns DRM_OK.  Asynchronous on `stream`, never a host synchronisation.
 */
int64_t drm_forward_dynamics_derivatives_scratch_floats(const drm_walk *walk, int64_t B);
int64_t drm_forward_dynamics_derivatives_scratch_floats_aligned(const drm_walk *walk, int64_t B);
int drm_forward_dynamics_derivatives(const drm_walk *walk, const float *q, const float *qd, const float *f, int64_t B, int32_t flags,
                                     float *qdd, float *dq, float *dqd, float *minv, float *scratch, void *stream);

/*
 * The inverse-dynamics regressor in one call (additive to ABI 15).  Inverse dynamics is linear in the inertial parameters: with
 * phi the stacked per-op (m, m c, I_o) — what ops_f holds at DRM_OPF_MASS / DRM_OPF_MCOM / DRM_OPF_IO — tau = Y(q, qd, qdd) phi.
 * What least-squares and recursive identification, adaptive (Slotine-Li) control and excitation-trajectory design need per sample,
 * and what a caller otherwise gets from 10 n_ops calls of drm_rnea on unit-parameter copies of the robot.
 *   q, qd, qdd [B, n] (qdd may be NULL: zeros)  ->  Y [B, n, P], dense, P = 10 n_ops (+ n with DRM_RNEA_DAMPING)
 *   Block i = columns 10 i .. 10 i + 9 belongs to op i of the walk, in walk order, and multiplies
 *       [m, m c_x, m c_y, m c_z, Ixx, Ixy, Ixz, Iyy, Iyz, Izz]
 *   of that op's link: c and I in the link's own URDF frame (the signed permutation of DRM_OPI_PERM is undone as the columns are
 *   stored), I about the frame's origin (I_c + m S(c) S(c)^T), an off-diagonal column the coefficient of the tied pair Iab = Iba.
 *   Y[b, j, block i] is zero where op i is not in the sub-tree of joint j, and everywhere for the ops of the static prefix; the zeros
 *   are written.  With DRM_RNEA_DAMPING Y[b, j, 10 n_ops + j] = qd_j (zero elsewhere): the last n parameters are the joint dampings
 *   in DoF order.  DRM_RNEA_GRAVITY: the base acceleration (0, 0, +9.81) of drm_rnea.
 *   Y phi = drm_rnea(q, qd, qdd) with the same flags, up to float32 rounding.
 * Serial 7-DoF arm chains (DRM_WALK_ARM_CHAIN, capacity 8), full 64-row tiles, 16-byte aligned q / qd / qdd / Y and table: ONE
 * kernel, a block of four wavefronts per tile, one row per lane, the blocks in registers, the tile of Y assembled in LDS and stored
 * whole in 16-byte stores (84 B in, 1 960 B out per row, nothing else through HBM).  Every other walk, the ragged tail, misaligned
 * pointers and DRM_REGRESSOR_COMPOSED: one hipMemsetAsync of those rows of Y, then one lane per row and a loop over the ops that
 * stores the rows of a body's ancestors.  A row with a non-finite q / qd / qdd gets non-finite entries wherever Y depends on that
 * input and changes no bit of any other row.
 *   scratch   drm_rnea_regressor_scratch_floats_aligned floats when q / qd / qdd / Y are 16-byte aligned,
 *             drm_rnea_regressor_scratch_floats floats otherwise and with DRM_REGRESSOR_COMPOSED: the rows' records between ops where
 *             64 rows of them do not fit the general kernel's LDS budget (3 n_ops + 12 n_slots floats per row and at most 2 048 tiles
 *             of 64 rows at a time; 0 for walks of up to 26 ops without branch points — arms, hands: scratch may then be NULL)
 * DRM_ERR_UNSUPPORTED for a walk whose rows of Y have 2^24 entries or more (n (10 n_ops + n)); DRM_ERR_INVALID for a NULL q / qd / Y
 * or a negative B; B == 0 returns DRM_OK.  Asynchronous on `stream`, never a host synchronisation, no allocation.
 */
int64_t drm_rnea_regressor_scratch_floats(const drm_walk *walk, int64_t B);
int64_t drm_rnea_regressor_scratch_floats_aligned(const drm_walk *walk, int64_t B);
int drm_rnea_regressor(const drm_walk *walk, const float *q, const float *qd, const float *qdd, int64_t B, int32_t flags, float *Y,
                       float *scratch, void *stream);

/*
 * The terms of  H(q) qdd + C(q, qd) qd + g(q) = tau  in one call (additive to ABI 15): the joint-space inertia matrix, the Coriolis
 * matrix and the gravity torques.  What passivity-based and adaptive control (tau = H a + C v + g - K s, v != qd), generalised-momentum
 * observers (pdot = tau + C^T qd - g + tau_ext, p = H qd) and Lagrangian model learning need, and what a caller otherwise gets from
 * dH/dq by n (n + 1) / 2 backward passes through drm_crba.
 *   q, qd [B, n]  ->  H [B, n, n], C [B, n, n], g [B, n]; any of the three may be NULL (not computed where that is cheap, not stored)
 *   H   what drm_crba returns, up to float32 rounding; symmetric to the bit
 *   g   drm_rnea(q, 0, 0, DRM_RNEA_GRAVITY): the torques that hold the robot still under the base acceleration (0, 0, +9.81)
 *   C   the CHRISTOFFEL matrix, C[i, j] = sum_k Gamma_ijk qd_k, Gamma_ijk = (dH_ij/dq_k + dH_ik/dq_j - dH_jk/dq_i) / 2: the one C with
 *       C qd + g = drm_rnea(q, qd, 0, DRM_RNEA_GRAVITY) for which dH/dt = C + C^T (dH/dt - 2 C skew-symmetric).  Joint damping is not
 *       part of C: tau = H qdd + C qd + g + damping * qd.
 *   H[i, j] and C[i, j] are exact zeros where joints i and j lie on different branches; the zeros are written.
 * One sweep over the tree (Echeandia and Wensing 2021, csrc/drm_lagrangian.hpp), every quantity in its link's own frame.  Serial 7-DoF
 * arm chains (DRM_WALK_ARM_CHAIN, capacity 8), full 64-row tiles, 16-byte aligned q / qd / H / C / g and table: ONE kernel, one
 * wavefront per tile, one row per lane, everything in registers, the tiles of H, C and g assembled in LDS and stored whole in 16-byte
 * stores (56 B in, 420 B out per row, nothing else through HBM; with H and g NULL 196 B out and neither is formed).  Every other walk,
 * the ragged tail, misaligned pointers and DRM_LAGRANGIAN_COMPOSED: one hipMemsetAsync of those rows of H and of C, then one lane per
 * row and two loops over the ops that store the entries between a joint and its ancestors.  A walk that carries its robot's own code
 * object runs these library kernels all the same.
 * A row with a q or qd that is not finite, or with a |q| beyond 1e5 (float32 no longer resolves such an angle), gets NaN in every
 * entry that is written and changes no bit of any other row.
 *   scratch   drm_lagrangian_dynamics_scratch_floats_aligned floats when q / qd / H / C / g are 16-byte aligned,
 *             drm_lagrangian_dynamics_scratch_floats floats otherwise and with DRM_LAGRANGIAN_COMPOSED: the rows' records between the
 *             sweeps where 64 rows of them do not fit the general kernel's LDS budget (12 n_ops + 22 n_slots floats per row and at
 *             most 2 048 tiles of 64 rows at a time; 0 for chains of up to 10 ops: scratch may then be NULL)
 * DRM_ERR_INVALID for a NULL q / qd, for H, C and g all NULL, or a negative B; B == 0 returns DRM_OK.  Asynchronous on `stream`, never
 * a host synchronisation, no allocation.
 */
int64_t drm_lagrangian_dynamics_scratch_floats(const drm_walk *walk, int64_t B);
int64_t drm_lagrangian_dynamics_scratch_floats_aligned(const drm_walk *walk, int64_t B);
int drm_lagrangian_dynamics(const drm_walk *walk, const float *q, const float *qd, int64_t B, int32_t flags, float *H, float *C, float *g,
                            float *scratch, void *stream);

/*
 * Inverse dynamics and its first-order derivatives in one call (additive to ABI 15): tau = ID(q, qd, qdd) and the partial derivatives
 * of tau with respect to q, qd and qdd.  What inverse-dynamics trajectory optimisation needs at every knot, and gain design for
 * computed-torque control, an EKF with a torque measurement and Gauss-Newton identification in the state; what a caller otherwise gets
 * from n backward passes through drm_rnea with one-hot cotangents plus drm_crba.
 *   q, qd, qdd [B, n]  ->  tau [B, n], dtau_dq [B, n, n], dtau_dqd [B, n, n], H [B, n, n];  [b, i, j] = d tau_i / d x_j;
 *   any of the four may be NULL (not stored; not formed where that is cheap)
 *   tau        what drm_rnea returns with the same DRM_RNEA_GRAVITY / DRM_RNEA_DAMPING flags, up to float32 rounding
 *   H          d tau / d qdd: what drm_crba returns, up to float32 rounding; symmetric to the bit
 *   dtau_dqd   with DRM_RNEA_DAMPING it includes diag(damping); gravity never enters it
 *   dtau_dq    damping never enters it
 *   Entries of the three matrices are exact zeros where joints i and j lie on different branches; the zeros are written.
 * One sweep out and one back over the tree (Carpentier and Mansard 2018; Singh, Russell and Wensing 2022; csrc/drm_idd.hpp), every
 * quantity in its link's own frame, O(n depth) work.  Serial 7-DoF arm chains (DRM_WALK_ARM_CHAIN, capacity 8), full 64-row tiles,
 * 16-byte aligned pointers and table: ONE kernel, one wavefront per tile, one row per lane, everything in registers, the tiles of the
 * outputs assembled in LDS and stored whole in 16-byte stores (84 B in, 616 B out per row, nothing else through HBM).  Every other walk,
 * the ragged tail, misaligned pointers and DRM_IDD_COMPOSED: one hipMemsetAsync of those rows of each matrix, then one lane per row and
 * two loops over the ops that store the entries between a joint and its ancestors.  A walk that carries its robot's own code object
 * runs these library kernels all the same.
 * A row with a q, qd or qdd that is not finite, or with a |q| beyond 1e5 (float32 no longer resolves such an angle), gets NaN in every
 * entry that is written and changes no bit of any other row.
 *   scratch   drm_rnea_derivatives_scratch_floats_aligned floats when every pointer is 16-byte aligned,
 *             drm_rnea_derivatives_scratch_floats floats otherwise and with DRM_IDD_COMPOSED: the rows' records between the sweeps
 *             where 64 rows of them do not fit the general kernel's LDS budget (15 n_ops + 28 n_slots floats per row and at most
 *             2 048 tiles of 64 rows at a time; 0 for chains of up to 8 ops: scratch may then be NULL)
 * DRM_ERR_INVALID for a NULL q / qd / qdd, for all four outputs NULL, or a negative B; B == 0 returns DRM_OK.  Asynchronous on
 * `stream`, never a host synchronisation, no allocation.
 */
int64_t drm_rnea_derivatives_scratch_floats(const drm_walk *walk, int64_t B);
int64_t drm_rnea_derivatives_scratch_floats_aligned(const drm_walk *walk, int64_t B);
int drm_rnea_derivatives(const drm_walk *walk, const float *q, const float *qd, const float *qdd, int64_t B, int32_t flags, float *tau,
                         float *dtau_dq, float *dtau_dqd, float *H, float *scratch, void *stream);

/*
 * The Lagrangian's own terms in one call (additive to ABI 15): the kinetic energy, the potential energy, the generalised momentum and
 * the gradients of both energies.  What energy-shaping and swing-up control, Hamiltonian / symplectic integration (qdot = dHam/dp,
 * pdot = -dHam/dq + tau), Lagrangian and Hamiltonian network losses and an energy-drift check of a rollout need, and what a caller
 * otherwise composes from drm_lagrangian_dynamics (420 B per row), two products, all-links forward kinematics and the link masses.
 *   q, qd [B, n]  ->  T [B], V [B], p [B, n], dT_dq [B, n], g [B, n]; any of the five may be NULL (not stored; with p, dT_dq and g all
 *   NULL the sweep back is not made)
 *   T       1/2 qd^T H(q) qd, formed as the sum over the bodies of 1/2 v_i . (I_i v_i) in each link's own frame, not via H
 *   V       9.81 sum_i m_i z_i, z_i the height of body i's centre of mass above the base frame's z = 0 plane, over the bodies of the
 *           walk that a joint moves.  The base and whatever is fixed to it are left out: they add a constant to V and nothing else.
 *   p       dT/dqd = H qd:  p_j = S_j . hC_j, hC_j the spatial momentum of joint j's sub-tree in link j's frame
 *   dT_dq   1/2 qd^T (dH/dq_j) qd = (C^T qd)_j with drm_lagrangian_dynamics' C:  -S_j . (v_j x* hC_j), no acceleration sweep
 *   g       dV/dq: drm_lagrangian_dynamics' g up to float32 rounding
 *   Joint damping enters none of them.
 * One sweep out (velocity, base acceleration, height) and one back (a 6-float momentum and a 4-float mass / first moment) over the
 * tree (csrc/drm_energy.hpp), every quantity in its link's own frame.  Serial 7-DoF arm chains (DRM_WALK_ARM_CHAIN, capacity 8), full
 * 64-row tiles, 16-byte aligned q / qd / p / dT_dq / g and table: ONE kernel, one wavefront per tile, one row per lane, everything in
 * registers, T and V one float per lane, the three [64, 7] tiles assembled in LDS and stored whole in 16-byte stores (56 B in, 92 B
 * out per row).  Every other walk, the ragged tail, misaligned pointers and DRM_ENERGY_COMPOSED: one lane per row and two loops over
 * the ops.  A walk that carries its robot's own code object runs these library kernels all the same.
 * A row with a q or qd that is not finite, or with a |q| beyond 1e5 (float32 no longer resolves such an angle), gets NaN in every
 * output that is written and changes no bit of any other row.
 *   scratch   drm_energy_scratch_floats_aligned floats when q / qd / p / dT_dq / g are 16-byte aligned, drm_energy_scratch_floats floats
 *             otherwise and with DRM_ENERGY_COMPOSED: the rows' records between the sweeps where 64 rows of them do not fit the general
 *             kernel's LDS budget (14 n_ops + 10 n_slots floats per row and at most 2 048 tiles of 64 rows at a time; 0 for chains of
 *             up to 9 ops: scratch may then be NULL)
 * DRM_ERR_INVALID for a NULL q / qd, for all five outputs NULL, or a negative B; B == 0 returns DRM_OK.  Asynchronous on `stream`,
 * never a host synchronisation, no allocation.
 */
int64_t drm_energy_scratch_floats(const drm_walk *walk, int64_t B);
int64_t drm_energy_scratch_floats_aligned(const drm_walk *walk, int64_t B);
int drm_energy(const drm_walk *walk, const float *q, const float *qd, int64_t B, int32_t flags, float *T, float *V, float *p, float *dT_dq,
               float *g, float *scratch, void *stream);

/*
 * Positions, velocities and classical accelerations of T links in ONE call (ABI 15, additive), and the joint torques of external
 * wrenches on T links in ONE call: what a caller otherwise composes from one drm_fk_jacobian launch and two small products PER LINK
 * (168 B per row of Jacobian, thrown away after one product).  `walk` is a MANY-TARGET FK walk (flatten.build_walk(targets=...), what
 * drm_fk takes): target t is the op whose DRM_OPI_OUT == t, fixed links that are targets are ops of their own, parents are
 * DRM_OPI_W1's.  The dynamics walk is not taken: it folds fixed links away.
 * Frame: drm_fk_jacobian's — WORLD axes, at the link frame's origin.  With lin_jac_t / ang_jac_t that call's outputs for link t:
 *   pos      [B, T, 3]  the link origin (drm_fk's position up to float32 rounding)
 *   lin_vel  [B, T, 3]  lin_jac_t qd                   ang_vel  [B, T, 3]  ang_jac_t qd
 *   lin_acc  [B, T, 3]  d/dt lin_vel = lin_jac_t qdd + d(lin_jac_t)/dt qd, the classical acceleration of the origin; gravity is NOT
 *                       included                        ang_acc  [B, T, 3]  d/dt ang_vel
 *   tau      [B, n]     sum_t lin_jac_t^T force[:, t] + ang_jac_t^T torque[:, t]; a force acts at the link ORIGIN (a force at another
 *                       point is the caller's torque += r x f).  Columns of DoFs that no target's chain crosses are written as zeros.
 * One world-frame sweep outwards (csrc/drm_links.hpp), for the torques followed by one inwards.  The two are adjoint:
 * sum_t force_t . lin_vel_t + torque_t . ang_vel_t == tau . qd for every qd, so each is the other's reverse mode.  By linearity
 * tau = drm_rnea(q, qd, qdd) - tau_ext balances external wrenches and qdd = drm_forward_dynamics(q, qd, f + tau_ext) applies them.
 *   drm_link_motion        q [B, n]; qd NULL => zero (positions alone), qdd NULL => zero (accelerations = Jdot qd); any of the five
 *                          outputs may be NULL, not all.  With both acceleration outputs NULL the acceleration terms are not formed,
 *                          with the velocity outputs NULL too neither are the velocity terms.
 *   drm_external_torques   force, torque [B, T, 3], either NULL (= zero), not both; tau [B, n]
 * A serial 7-DoF arm chain of 8 ops (DRM_WALK_ARM_CHAIN, capacity 8) whose 8 ops are all targets in walk order
 * (DRM_WALK_TARGETS_ORDERED, n_targets == 8), full 64-row tiles, 16-byte aligned pointers and table: fused kernels, one wavefront per
 * tile, one row per lane, everything in registers, every tile through LDS in 16-byte accesses (84 B in, up to 480 B out per row; 220 B
 * in, 28 B out).  Every other walk (trees, hands, prismatic joints, two-op skew-axis links, target subsets), the ragged tail,
 * misaligned pointers and DRM_LINKS_COMPOSED: one lane per row, loops over the ops.
 * A row with a q, qd or qdd that is not finite, or with a |q| beyond 1e5, is walked at rest at q = 0, gets NaN in every output that is
 * written and changes no bit of any other row.  A wrench component that is not finite makes the torques of that link's ancestor
 * joints non-finite and changes nothing else.
 *   scratch   the matching _scratch_floats query's floats (the _aligned form returns the same): the rows' state where 64 rows of it do
 *             not fit the general kernels' LDS budget — motion 24 floats per branch point, torques 12 n_ops + 24 n_slots floats per
 *             row, at most 2 048 tiles of 64 rows at a time; 0 (scratch may be NULL) for drm_link_motion of walks of up to 5 branch
 *             points and for drm_external_torques of chains of up to 10 ops
 * DRM_ERR_INVALID for a NULL q, no output (no wrench input; a NULL tau), a negative B, or an n_targets that cannot be the walk's number
 * of output slots (outside [1, n_ops]; slots beyond n_targets are neither read nor written); B == 0 returns DRM_OK.  Asynchronous on
 * `stream`, never a host synchronisation, no allocation.
 */
#define DRM_LINKS_COMPOSED 1024     /* force the general kernel on every row (tests, A/B) */
int64_t drm_link_motion_scratch_floats(const drm_walk *walk, int64_t B);
int64_t drm_link_motion_scratch_floats_aligned(const drm_walk *walk, int64_t B);
int64_t drm_external_torques_scratch_floats(const drm_walk *walk, int64_t B);
int64_t drm_external_torques_scratch_floats_aligned(const drm_walk *walk, int64_t B);
int drm_link_motion(const drm_walk *walk, const float *q, const float *qd, const float *qdd, int64_t B, int32_t n_targets, int32_t flags,
                    float *pos, float *lin_vel, float *ang_vel, float *lin_acc, float *ang_acc, float *scratch, void *stream);
int drm_external_torques(const drm_walk *walk, const float *q, const float *force, const float *torque, int64_t B, int32_t n_targets,
                         int32_t flags, float *tau, float *scratch, void *stream);

/*
 * The q-gradient of both link sweeps in one call (additive to ABI 15).  The two are the two sides of one scalar, the power of the
 * wrenches,
 *   S(q; qd, force, torque) = sum_t force_t . lin_vel_t + torque_t . ang_vel_t = tau(q; force, torque) . qd,
 * so dS/dq with qd, force and torque held fixed is the q-gradient of drm_link_motion's velocities under the cotangents
 * (force, torque) := (g_lin_vel, g_ang_vel), and the q-gradient of drm_external_torques under the cotangent qd := g_tau.  No
 * kinematic Hessian is formed: the two sweeps of drm_external_torques with the velocities carried outwards and one more 3-vector
 * carried inwards (csrc/drm_links.hpp link_power_dq_walk).
 *   dq   [B, n]  dS/dq.  Columns of DoFs that no target's chain crosses are written as zeros.
 *   tau  [B, n]  optional (NULL: not stored): drm_external_torques' output on the same q, force and torque, to the bit — the backward
 *                of the velocities gets grad_q and grad_qd from one launch.
 * walk, q, force, torque, n_targets, flags (DRM_LINKS_COMPOSED), scratch and stream: drm_external_torques'; qd [B, n] must be given.
 * The same two kernels: fused for the arm chain of 8 targets on full 64-row tiles with every pointer 16-byte aligned (q, qd, the two
 * wrench tiles in and dq, tau out through LDS in 16-byte accesses: 248 B in, 28 or 56 B out per row), one lane per row over the ops
 * elsewhere.  A row with a q or qd that is not finite, or with a |q| beyond 1e5, gets NaN in dq and tau and changes no bit of any
 * other row.  A wrench component that is not finite makes the dq and tau entries of that link's ancestor joints non-finite and
 * changes nothing else.
 *   scratch   drm_link_power_dq_scratch_floats' floats (the _aligned form returns the same): the rows' state where 64 rows of it do
 *             not fit the general kernel's LDS budget — 21 n_ops + 24 n_slots floats per row, at most 2 048 tiles of 64 rows at a
 *             time; 0 (scratch may be NULL) for chains of up to 6 ops
 * DRM_ERR_INVALID for a NULL q, qd or dq, no wrench input, a negative B or an n_targets outside [1, n_ops]; B == 0 returns DRM_OK.
 * Asynchronous on `stream`, never a host synchronisation, no allocation.
 */
int64_t drm_link_power_dq_scratch_floats(const drm_walk *walk, int64_t B);
int64_t drm_link_power_dq_scratch_floats_aligned(const drm_walk *walk, int64_t B);
int drm_link_power_dq(const drm_walk *walk, const float *q, const float *qd, const float *force, const float *torque, int64_t B,
                      int32_t n_targets, int32_t flags, float *dq, float *tau, float *scratch, void *stream);

/*
 * Contact: spheres on the links against ONE plane (a penalty spring-damper with regularised Coulomb friction) and spring-dampers at the
 * joint limits, as joint torques of one state (drm_contact_torques) and inside a rollout (drm_contact_rollout), where they depend on
 * the state of every step and so cannot be handed to drm_forward_dynamics_rollout in advance.  The law (csrc/drm_contact.hpp), with
 * p, v, w drm_link_motion's origin, linear and angular velocity of a contact link, rl its radius, n the unit normal (`normal` is
 * normalised in double by the call), d = offset, k = stiffness, c = damping, mu = friction, c_t = friction_slope:
 *   r = -rl n     depth = rl - (n.p - d)     v_c = v + w x r     v_n = n.v_c     v_t = v_c - v_n n
 *   f_n = max(0, k depth - c v_n) if depth > 0, else 0          f_t = -min(c_t, mu f_n / |v_t|) v_t  (0 when mu, c_t, f_n or |v_t| is 0)
 *   force = f_n n + f_t     moment = r x force     tau_ext = sum_t lin_jac_t^T force_t + ang_jac_t^T moment_t
 *   q_j < lower_j:  tau_lim_j = k_l (lower_j - q_j) - c_l qd_j;   q_j > upper_j:  tau_lim_j = -k_l (q_j - upper_j) - c_l qd_j;   else 0
 *   drm_contact_torques   tau [B, n] = tau_ext + tau_lim; force, moment [B, n_targets, 3] (either may be NULL: not stored)
 *   drm_contact_rollout   drm_forward_dynamics_rollout with qdd_t = FD(q_t, qd_t, tau[t] + tau_ext(q_t, qd_t) + tau_lim(q_t, qd_t))
 * `links_walk` is the many-target FK walk drm_link_motion takes and its n_targets the contact links; `dyn_walk` the dynamics walk of
 * the same robot.  `plane` NULL: no contact (then springs must be given).  `radius`: DEVICE pointer to n_targets floats, or NULL = 0.
 * `springs` NULL: no joint-limit springs; else lower / upper are DEVICE pointers to n floats (-inf / +inf: a free DoF).  flags:
 * DRM_RNEA_GRAVITY, DRM_RNEA_DAMPING, DRM_ROLLOUT_EXPLICIT_EULER with drm_forward_dynamics_rollout's meaning, DRM_LINKS_COMPOSED.
 * A links_walk that drm_link_motion runs fused (7-DoF arm chain of 8 ops, all targets in walk order; for the rollout also a dyn_walk
 * that drm_forward_dynamics_rollout's arm kernel takes), full 64-row tiles, 16-byte aligned pointers and tables (rollout: slabs too,
 * B n % 4 == 0): ONE launch, one wavefront per tile, one row per lane, state in registers across the steps.  Everything else is
 * composed on the caller's stream out of the one scratch: drm_link_motion -> one element-wise law kernel -> drm_external_torques ->
 * one add of the springs (and of tau[t]); per rollout step followed by drm_forward_dynamics and the integrator kernel.
 * A row of drm_contact_torques with a q or qd that is not finite (|q| beyond 1e5) gets NaN in every output; a row of a rollout with a
 * non-finite q0, qd0 or tau gets non-finite outputs from that step on.  Neither changes a bit of any other row.
 * DRM_ERR_INVALID: a NULL required pointer, T < 1, a dt that is not finite and positive, a plane or spring parameter that is not
 * finite or is negative, a zero normal, B < 0, neither plane nor springs; B == 0 returns DRM_OK.  Asynchronous on `stream`, no
 * allocation, never a host synchronisation.
 */
typedef struct drm_contact_plane {
    float normal[3], offset, stiffness, damping, friction, friction_slope;
} drm_contact_plane;
typedef struct drm_joint_springs {
    float stiffness, damping;
} drm_joint_springs;
int64_t drm_contact_torques_scratch_floats(const drm_walk *links_walk, int64_t B);
int64_t drm_contact_torques_scratch_floats_aligned(const drm_walk *links_walk, int64_t B);
int64_t drm_contact_rollout_scratch_floats(const drm_walk *dyn_walk, const drm_walk *links_walk, int64_t B);
int64_t drm_contact_rollout_scratch_floats_aligned(const drm_walk *dyn_walk, const drm_walk *links_walk, int64_t B);
int drm_contact_torques(const drm_walk *links_walk, const float *q, const float *qd, int64_t B, int32_t n_targets,
                        const drm_contact_plane *plane, const float *radius, const drm_joint_springs *springs, const float *lower,
                        const float *upper, int32_t flags, float *tau, float *force, float *moment, float *scratch, void *stream);
int drm_contact_rollout(const drm_walk *dyn_walk, const drm_walk *links_walk, const float *q0, const float *qd0, const float *tau,
                        int64_t B, int32_t T, float dt, int32_t flags, int32_t n_targets, const drm_contact_plane *plane,
                        const float *radius, const drm_joint_springs *springs, const float *lower, const float *upper, float *q_traj,
                        float *qd_traj, float *qdd_traj, float *scratch, void *stream);

/*
 * The vector-Jacobian product of drm_contact_torques in one call (additive to ABI 15): with tau_c(q, qd) that call's tau and grad_tau
 * [B, n] a cotangent on it,
 *   grad_q   [B, n]  d/dq  (grad_tau . tau_c)          grad_qd  [B, n]  d/dqd (grad_tau . tau_c)
 * either may be NULL (not stored), not both; the other's bits do not depend on it.  No Jacobian and no kinematic Hessian is formed.
 * With (a_t, b_t) = (lin_jac_t grad_tau, ang_jac_t grad_tau) the cotangents of the wrenches and (gp_t, gv_t, gw_t) the law's backward
 * of them onto (p_t, v_t, w_t) (csrc/drm_contact.hpp contact_wrench_vjp):
 *   grad_qd = drm_external_torques(q, gv, gw) - c_l grad_tau_j on an active spring
 *   grad_q  = drm_link_power_dq(q, grad_tau, force, moment) + drm_external_torques(q, gp, 0) + drm_link_power_dq(q, qd, gv, gw)
 *             - k_l grad_tau_j on an active spring
 * The law is piecewise smooth: where depth, k depth - c v_n, c_t |v_t| - mu f_n, q - lower or upper - q changes sign the derivative is
 * that of the branch drm_contact_torques takes at (q, qd); an exact tie of the two friction branches goes to the viscous one.
 * links_walk, q, qd, n_targets, plane, radius, springs, lower, upper, flags (DRM_LINKS_COMPOSED), stream: drm_contact_torques', except
 * that `plane` may be NULL when springs are given (the springs' share alone).  The same two forms: the 7-DoF arm chain of 8 ops, all
 * targets in walk order, on full 64-row tiles with every pointer 16-byte aligned runs ONE launch, one row per lane — one sweep outwards
 * that carries the velocities at rates qd and at rates grad_tau together with the law and its backward per link, one sweep inwards
 * with the three wrench sets above, the two [64, 7] tiles out through LDS in 16-byte stores (84 B in, 56 B out per row).  Everything
 * else, the B % 64 tail included, is composed on the caller's stream out of the one scratch: drm_link_motion twice (rates qd, rates
 * grad_tau), one element-wise kernel for the law and its backward, drm_link_power_dq twice, drm_external_torques once, one add.
 * A row whose q, qd or grad_tau is not finite (|q| beyond 1e5) gets NaN in both outputs and changes no bit of any other row.
 *   scratch   drm_contact_torques_vjp_scratch_floats' floats (the _aligned form returns the same): the composed form over all B rows
 * DRM_ERR_INVALID: a NULL q, qd or grad_tau, both outputs NULL, a plane or spring parameter that is not finite or is negative, a zero
 * normal, B < 0, an n_targets outside [1, n_ops], neither plane nor springs; B == 0 returns DRM_OK.  Asynchronous on `stream`, no
 * allocation, never a host synchronisation.
 */
int64_t drm_contact_torques_vjp_scratch_floats(const drm_walk *links_walk, int64_t B);
int64_t drm_contact_torques_vjp_scratch_floats_aligned(const drm_walk *links_walk, int64_t B);
int drm_contact_torques_vjp(const drm_walk *links_walk, const float *q, const float *qd, const float *grad_tau, int64_t B,
                            int32_t n_targets, const drm_contact_plane *plane, const float *radius,
                            const drm_joint_springs *springs, const float *lower, const float *upper, int32_t flags,
                            float *grad_q, float *grad_qd, float *scratch, void *stream);

/*
 * Collision: spheres fixed to the links against a world of spheres and oriented boxes shared by the whole batch, and against each
 * other through a list of sphere pairs (additive to ABI 15).  One call gives the cost and its q-gradient (drm_collision_cost) or the
 * sphere centres and their clearances (drm_sphere_distances).  The law (csrc/drm_collision.hpp), in float32 on explicit fused
 * multiply-adds; x_s = p_l + R_l c_s the world centre of sphere s on link l, r_s its radius:
 *   sphere obstacle (c, r)   sd = |x - c| - r, direction (x - c) / |x - c| (0 when the norm is 0)
 *   box (c, Rb, h)           y = Rb^T (x - c), a = |y| - h; outside (max a > 0) sd = |max(a, 0)|, direction Rb (sign(y) max(a, 0) / sd);
 *                            inside sd = max a, direction Rb (sign(y_i) e_i) with i the first index at which a is largest
 *   d_sm = sd_m(x_s) - r_s                        d_ij = |x_i - x_j| - r_i - r_j
 *   phi(u) = 0 (u <= 0), u^2 / (2 eta) (0 < u <= eta), u - eta / 2 (above); u = eta - d; phi' = clamp(u / eta, 0, 1)
 *   cost = world_weight sum_{s, m} phi(world_activation - d_sm) + self_weight sum_pairs phi(self_activation - d_ij)
 *   dq   = sum_l lin_jac_l^T F_l + ang_jac_l^T M_l,  F_l = sum_{s on l} dcost/dx_s,  M_l = sum_{s on l} (x_s - p_l) x dcost/dx_s
 *   world_distance_s = min_m d_sm (+inf with an empty world)      self_distance_s = min over the pairs containing s (+inf without one)
 * `links_walk` / n_targets: the many-target FK walk drm_link_motion takes.
 *   drm_collision_spheres   spheres: DEVICE [S, 4] = centre in the STORED frame of the link's op (R~ = R P of DRM_OPI_PERM: c~ = P^T c; a
 *                           link of two ops takes the frame of its last op) and radius, grouped by link: the root's group first (R = I,
 *                           p = 0: a constant of the cost, nothing in dq, but they take part in pairs), then the targets in order.
 *                           start: DEVICE [n_targets + 2] CSR offsets of the groups, start[0] = 0, start[n_targets + 1] = n_spheres;
 *                           empty groups are allowed.
 *   drm_collision_world     spheres: DEVICE [n_spheres, 4] = centre, radius; boxes: DEVICE [n_boxes, 16] = centre 3, half extents 3,
 *                           rotation 9 row-major (box -> world), one pad.  Either may be empty.
 *   drm_collision_pairs     pairs: DEVICE [n_pairs, 2] indices into the grouped sphere order, i != j.
 *   drm_collision_cost      cost [B], dq [B, n]: either may be NULL, not both; with dq NULL no sweep inwards runs.  world or pairs may be
 *                           NULL, not both.
 *   drm_sphere_distances    center [B, S, 3], world_distance [B, S], self_distance [B, S] in the grouped order: any may be NULL, not
 *                           all; an output whose input is NULL is filled with +inf.
 * A links_walk that drm_link_motion runs fused (7-DoF arm chain of 8 ops, all 8 targets in walk order), full 64-row tiles, 16-byte
 * aligned pointers, n_spheres <= 64, obstacles <= 32 and n_pairs <= 1 024: ONE launch, one row per lane, a block of wavefronts per
 * 64-row tile that share the centres in LDS.  Everything else (trees, hands, prismatic and skew joints, link subsets, ragged tails,
 * misaligned pointers, anything over the caps, DRM_LINKS_COMPOSED): one lane per row on the caller's stream out of the one scratch — a
 * walk outwards with the world terms, the pairs, then drm_external_torques for dq.  Order of every sum: spheres in grouped order
 * against the obstacles in table order, spheres before boxes, then the pairs in list order; the two paths agree to rounding.
 * A row with a q that is not finite, or with a |q| beyond 1e5, is walked at q = 0, gets NaN in every output that is written and
 * changes no bit of any other row.
 *   scratch   the matching _scratch_floats query's floats over ALL B rows of the general path, whatever the alignment, the targets and
 *             the caps: per row the centres (3 n_spheres), the link origins and wrenches (9 n_ops), the cost, plus the state of the
 *             walk outwards and of drm_external_torques.  The _aligned form is for a call without DRM_LINKS_COMPOSED whose pointers
 *             are all 16-byte aligned; told n_targets and the sizes of the tables (n_obstacles = world spheres + boxes), it returns
 *             the floats of the B % 64 tail rows alone where the fused kernel takes the full tiles (which needs none: scratch may be
 *             NULL when the query returns 0), and of all B rows otherwise.
 * DRM_ERR_INVALID: a NULL required pointer, B < 0, an n_targets outside [1, n_ops], n_spheres < 1, a negative count, neither world nor
 * pairs (drm_collision_cost), no output, an activation that is not finite and positive where its term is present, a weight that is
 * negative or not finite; B == 0 returns DRM_OK.  Asynchronous on `stream`, no allocation, never a host synchronisation.
 */
typedef struct drm_collision_spheres {
    const float *spheres;
    const int32_t *start;
    int32_t n_spheres;
} drm_collision_spheres;
typedef struct drm_collision_world {
    const float *spheres;
    const float *boxes;
    int32_t n_spheres, n_boxes;
} drm_collision_world;
typedef struct drm_collision_pairs {
    const int32_t *pairs;
    int32_t n_pairs;
} drm_collision_pairs;
typedef struct drm_collision_params {
    float world_weight, world_activation, self_weight, self_activation;
} drm_collision_params;
int64_t drm_collision_cost_scratch_floats(const drm_walk *links_walk, int64_t B, int32_t n_spheres);
int64_t drm_collision_cost_scratch_floats_aligned(const drm_walk *links_walk, int64_t B, int32_t n_targets, int32_t n_spheres,
                                                  int32_t n_obstacles, int32_t n_pairs);
int64_t drm_sphere_distances_scratch_floats(const drm_walk *links_walk, int64_t B, int32_t n_spheres);
int64_t drm_sphere_distances_scratch_floats_aligned(const drm_walk *links_walk, int64_t B, int32_t n_targets, int32_t n_spheres,
                                                    int32_t n_obstacles, int32_t n_pairs);
int drm_collision_cost(const drm_walk *links_walk, const float *q, int64_t B, int32_t n_targets, const drm_collision_spheres *spheres,
                       const drm_collision_world *world, const drm_collision_pairs *pairs, const drm_collision_params *params,
                       int32_t flags, float *cost, float *dq, float *scratch, void *stream);
int drm_sphere_distances(const drm_walk *links_walk, const float *q, int64_t B, int32_t n_targets, const drm_collision_spheres *spheres,
                         const drm_collision_world *world, const drm_collision_pairs *pairs, int32_t flags, float *center,
                         float *world_distance, float *self_distance, float *scratch, void *stream);

/*
 * Reverse-mode derivative of drm_fk: what torch autograd computes in the reference when a loss on
 * compute_forward_kinematics' outputs is back-propagated to q and to learnable `trans` / `rot_angles`
 * (robot_model.py:139-195, 223-248, 669-713; examples/learn_kinematics_of_iiwa.py:25-61).
 *   q          [B, n]        joint angles of the forward call
 *   grad_pos   [B, T, 3]     dL/dpos of every target
 *   grad_rot   [B, T, 3, 3]  dL/dR of every target's rotation matrix, or NULL.  The reference's quaternion is made of
 *                            entries of R copied inside autograd (spatial_vector_algebra.py:108-136; only its
 *                            normalisation is detached), so a loss on the quaternion is a loss on R: the host layer turns
 *                            dL/dquat into dL/dR (robot_model._quat_grad_to_rot), the kernel carries it through the chain
 *   param_mask               bit k set: produce the constant gradient of op k (its link is learnable)
 *   grad_q     [B, n]        dL/dq, or NULL
 *   grad_ops_f [capacity, DRM_OPF_STRIDE]  dL/dF at DRM_OPF_FIJ(i, j), dL/dt at DRM_OPF_TI(i), summed over the
 *                            batch in a fixed order (deterministic); zeros elsewhere.  NULL iff param_mask == 0.
 *   scratch    drm_fk_backward_scratch_floats(B, capacity) floats, owned by the caller
 * The walk must give every branch point its own save slot (flatten.WalkProgram.slots_unique).
 */
int64_t drm_fk_backward_scratch_floats(int64_t B, int32_t capacity);
int drm_fk_backward(const drm_walk *walk, const float *q, int64_t B, int32_t n_targets, const float *grad_pos,
                    const float *grad_rot, uint64_t param_mask, float *grad_q, float *grad_ops_f, float *scratch, void *stream);

/*
 * Reverse-mode derivative of drm_fk_jacobian: what torch autograd computes in the reference when a loss on
 * compute_endeffector_jacobian's outputs (and, optionally, on the target's position) is back-propagated to q and to
 * learnable `trans` / `rot_angles` (robot_model.py:626-667 on top of 139-195).  The walk is the root->link chain
 * drm_fk_jacobian takes (no branch points).
 *   grad_pos      [B, 3]      dL/dpos of the target, or NULL        grad_rot  [B, 3, 3]  dL/dR of the target, or NULL
 *   grad_lin_jac  [B, 3, n]   dL/dlin_jac      grad_ang_jac  [B, 3, n]   dL/dang_jac
 *   param_mask, grad_q, grad_ops_f, scratch (drm_fk_backward_scratch_floats)   as for drm_fk_backward
 */
int drm_fk_jacobian_backward(const drm_walk *walk, const float *q, int64_t B, const float *grad_pos, const float *grad_rot,
                             const float *grad_lin_jac, const float *grad_ang_jac, uint64_t param_mask, float *grad_q,
                             float *grad_ops_f, float *scratch, void *stream);

/*
 * One training step's worth of the reference's kinematics-learning loop in one pass over q
 * (examples/learn_kinematics_of_iiwa.py:47-55: compute_forward_kinematics (robot_model.py:223-248) -> torch.nn.MSELoss ->
 * backward through robot_model.py:139-195 with learnable `trans` / `rot_angles`, robot_model.py:669-713):
 *   loss[0]     = mean over the B x 3 entries of (pos(q) - target)^2, pos = position of the walk's target (its last op)
 *   grad_q      [B, n] or NULL   d loss / d q
 *   grad_ops_f  [capacity, DRM_OPF_STRIDE]  d loss / d (R_fixed, trans) of the ops in param_mask (as drm_fk_backward), NULL iff
 *               param_mask == 0
 *   target      [B, 3];  scratch: drm_fk_mse_scratch_floats(B, capacity) floats, owned by the caller
 * The chain is walked once per sample (the forward pose, the loss and the closed-form adjoints of drm_fk_backward's chain
 * kernel); the batch sums are reduced in a fixed order (bit-stable from run to run).  Two launches.
 * Takes serial 7-DoF arm chains (DRM_WALK_ARM_CHAIN, capacity 8: the iiwa of BASELINE configuration 5, the Panda), B a
 * multiple of 64, 16-byte aligned pointers; DRM_ERR_UNSUPPORTED otherwise (compose drm_fk + the loss + drm_fk_backward).
 */
int64_t drm_fk_mse_scratch_floats(int64_t B, int32_t capacity);
int drm_fk_mse(const drm_walk *walk, const float *q, const float *target, int64_t B, uint64_t param_mask, float *loss,
               float *grad_q, float *grad_ops_f, float *scratch, void *stream);

/*
 * ABI 12: drm_fk_mse for a walk WITH learnable links, from their URDF-level parameters to the gradients with respect to them —
 * what drm_walk_table -> drm_fk_mse -> drm_walk_table_backward compute (the whole forward + loss + backward of
 * examples/learn_kinematics_of_iiwa.py:47-55 with the parameter modules of rigid_body_params.py in the loop), in TWO launches
 * instead of five: every wavefront of the first launch rebuilds the rows of the learnable links itself (R_fixed = (Rz Ry) Rx of
 * rot_angles, rigid_body.py:138-143; trans), the second adds the rows of partial sums AND takes the result back through that map.
 *   walk->ops_f   the table of the CONSTANT links gathered into walk order (`base` of drm_walk_table)
 *   sel, gsign    [capacity * DRM_OPF_STRIDE] as for drm_walk_table: entry e of the table is element sel[e] % 32 of the link row of
 *                 learnable link sel[e] / 32, times gsign[e] (+-1: the axis canonicalisation), or the constant (sel[e] < 0)
 *   links         HOST array of n_links (1 .. DRM_FK_MSE_MAX_LINKS) structs of DEVICE pointers, one per learnable link: the outputs
 *                 of its parameter modules where they lie (no packing pass).  Forward kinematics reads rot_angles[3] and trans[3];
 *                 the other four may be NULL.
 *   grad_params   [n_links, 20] d loss / d (rot_angles, trans, mass, com, inertia_mat, damping) in drm_walk_table's layout (the last
 *                 14 of a link are zeros: forward kinematics does not depend on them)
 *   loss, grad_q, target, param_mask (!= 0: the ops of the learnable links), scratch (drm_fk_mse_scratch_floats): as for drm_fk_mse,
 *   and the same walks / batches / alignment; DRM_ERR_UNSUPPORTED otherwise (compose the three calls).  Sums in drm_fk_mse's and
 *   drm_walk_table_backward's order: the same bits as the composition.
 */
#define DRM_FK_MSE_MAX_LINKS 8
struct drm_link_pieces {
    const float *rot_angles, *trans, *mass, *com, *inertia_mat, *damping; /* 3, 3, 1, 3, 9, 1 floats */
};
int drm_fk_mse_links(const drm_walk *walk, const int32_t *sel, const float *gsign, const struct drm_link_pieces *links,
                     int32_t n_links, const float *q, const float *target, int64_t B, uint64_t param_mask, float *loss,
                     float *grad_q, float *grad_params, float *scratch, void *stream);

/*
 * Reverse-mode derivative of drm_rnea: what torch autograd computes in the reference when a loss on
 * compute_inverse_dynamics' torques is back-propagated to learnable link parameters and to q / qd / qdd
 * (robot_model.py:305-375, 669-713; examples/learn_dynamics_iiwa.py:49-96).
 *   q, qd, qdd [B, n], flags      the arguments of the forward call (qdd may be NULL = zeros)
 *   grad_tau   [B, n]             dL/dtau
 *   param_mask                    bit k set: produce the constant gradients of op k (its link is learnable)
 *   grad_q, grad_qd, grad_qdd [B, n]   all three or all NULL
 *   grad_ops_f [capacity, DRM_OPF_STRIDE]  gradient of every constant of the selected ops in the op-row layout
 *                                 (FT block, mass, mass*com, I_o, damping), summed over the batch in a fixed order;
 *                                 zeros elsewhere.  NULL iff param_mask == 0.
 *   scratch    drm_rnea_backward_scratch_floats(B, capacity, n_dofs, n_slots) floats, owned by the caller
 * The walk must give every branch point its own save slot (flatten.WalkProgram.slots_unique).
 */
int64_t drm_rnea_backward_scratch_floats(int64_t B, int32_t capacity, int32_t n_dofs, int32_t n_slots);
int drm_rnea_backward(const drm_walk *walk, const float *q, const float *qd, const float *qdd, int64_t B, int32_t flags,
                      const float *grad_tau, uint64_t param_mask, float *grad_q, float *grad_qd, float *grad_qdd,
                      float *grad_ops_f, float *scratch, void *stream);

/*
 * Link-table rows from URDF-level link parameters, and the derivative of that map, for the rows of LEARNABLE links
 * (what the reference recomputes from its parameter modules on every call: rigid_body.py:138-143 R_fixed,
 * spatial_vector_algebra.py:321-327 mcom and I_o, and differentiates with one autograd node per tiny op).
 *   params [n_links, 20]  rpy (3) trans (3) mass (1) com (3) inertia_mat (9, about the com) damping (1)
 *   rows   [n_links, 32]  F (9, row-major) t (3) mass mcom (3) I_o (9) damping 0...   (the host gathers these into
 *                         walk order; flatten._gather_row)
 */
int drm_link_rows(const float *params, int32_t n_links, float *rows, void *stream);
int drm_link_rows_backward(const float *params, const float *grad_rows, int32_t n_links, float *grad_params, void *stream);

/*
 * The walk table (ops_f) of a robot with learnable links in ONE launch, and the derivative of that map in another: what
 * the reference does implicitly by calling its parameter modules inside every per-link op (rigid_body.py:138-143,
 * spatial_vector_algebra.py:321-327) and differentiating through them.
 *   params   [n_links, 20]   URDF-level parameters of the learnable links (drm_link_rows layout), n_links <= 32
 *   base     [n_entries]     the walk table built from the constant links (entries of learnable links are ignored)
 *   sel      [n_entries]     int32: index into the flattened [n_links, 32] rows for entries that come from a learnable
 *                            link, -1 for entries taken from `base`
 *   gsign    [n_entries]     the exact +-1 factors of the axis canonicalisation (flatten.WalkProgram.gsign)
 *   ops_f    [n_entries]     out (n_entries = capacity * DRM_OPF_STRIDE)
 * drm_walk_table_backward: grad_ops_f [n_entries] -> grad_params [n_links, 20], summed in a fixed order.
 */
int drm_walk_table(const float *params, int32_t n_links, const float *base, const int32_t *sel, const float *gsign,
                   int32_t n_entries, float *ops_f, void *stream);
int drm_walk_table_backward(const float *params, int32_t n_links, const float *grad_ops_f, const int32_t *sel,
                            const float *gsign, int32_t n_entries, float *grad_params, void *stream);

/*
 * ABI 13: the walk table straight from the learnable links' parameter TENSORS, where they lie and in the form their modules store
 * them, and the derivative of that map back to those tensors — one launch each.  What the reference does by calling the parameter
 * modules inside every per-link op (rigid_body.py:138-143; rigid_body_params.py:26-43 PositiveScalar, :252-404 the inertia-matrix
 * modules) and differentiating through them with one autograd node per tiny op: a learn-dynamics step
 * (examples/learn_dynamics_iiwa.py:49-96) spends 14 + 1 + 21 launches there (l * l + min per link, the cat of 42 pieces, the
 * backward of the squares) around drm_walk_table's two.
 *   links  [n_links]   where rot_angles, trans, mass, com, inertia_mat, damping of a learnable link lie (device addresses; constant
 *                      pieces point at the constants).  A piece in a form other than DRM_FORM_PLAIN points at the module's RAW parameter:
 *                      one float for the scalars, l[6] = (diagonal entries, then (1,0), (2,0), (2,1)) for inertia_mat
 *   forms  [n_links]   the form of mass / inertia_mat / damping and its constant (min_val, bias); NULL = everything plain
 *   base, sel, gsign, n_entries, ops_f   as for drm_walk_table
 * drm_walk_table_links_backward: grad_ops_f [n_entries] -> grad_params [n_links, 20] in drm_link_rows' layout, with respect to what lies
 * AT THE ADDRESSES (the raw parameters; inertia_mat in a six-number form fills the first six of its nine places, zeros behind).
 * Sums in drm_walk_table_backward's order.  At most 32 links.
 */
#define DRM_FORM_PLAIN 0
#define DRM_FORM_SQUARE_PLUS 1 /* mass, damping: l * l + c */
#define DRM_FORM_SYMM 2        /* inertia_mat: symmetric from l[6] */
#define DRM_FORM_SPD 3         /* inertia_mat: L L^T + c E */
#define DRM_FORM_COV 4         /* inertia_mat: tr(S) E - S, S = L L^T + c E */
struct drm_link_forms {
    int32_t mass, inertia_mat, damping;
    float mass_c, inertia_mat_c, damping_c;
};
int drm_walk_table_links(const struct drm_link_pieces *links, const struct drm_link_forms *forms, int32_t n_links, const float *base,
                         const int32_t *sel, const float *gsign, int32_t n_entries, float *ops_f, void *stream);
int drm_walk_table_links_backward(const struct drm_link_pieces *links, const struct drm_link_forms *forms, int32_t n_links,
                                  const float *grad_ops_f, const int32_t *sel, const float *gsign, int32_t n_entries,
                                  float *grad_params, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DRM_HIP_H */
