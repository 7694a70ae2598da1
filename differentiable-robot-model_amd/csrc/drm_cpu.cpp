// drm_cpu.cpp — the HOST build of the C ABI (include/drm_hip.h) → libdrm_cpu.so: what a model constructed with device="cpu"
// (the reference's default, robot_model.py:100-104; its whole test suite builds models there,
// tests/test_kinematics_dynamics.py:133-137) computes with.  The per-sample arithmetic is the kernels' own (drm_sample.hpp /
// drm_tree.hpp through the loops of drm_host_loops.hpp) compiled by g++; rows are processed in CHUNK-row pieces that a small
// pool of threads picks up.  Same entry points, same argument meaning and error codes as libdrm_hip.so, with HOST pointers;
// `stream` is ignored (calls return when the results are written).
//
// NOT a fallback of the HIP path: the Python binding picks the library by the DEVICE OF THE MODEL (backend.library_for) —
// tensors on a HIP device only ever reach libdrm_hip.so, which must exist (backend.load_library raises otherwise).
//
// Batch sums of the backward entry points (grad_ops_f, the loss of drm_fk_mse): one partial per CHUNK rows, added up in chunk
// order in double — the result does not depend on the number of threads.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <limits>
#include <thread>
#include <vector>

#include "drm_host_loops.hpp"
#include "drm_link_forms.hpp"
#include "drm_ik.hpp"
#include "drm_osc.hpp"
#include "drm_fdd.hpp"
#include "drm_regressor.hpp"
#include "drm_lagrangian.hpp"
#include "drm_idd.hpp"
#include "drm_energy.hpp"
#include "drm_links.hpp"
#include "drm_contact.hpp"
#include "drm_collision.hpp"
#include "drm_rollout.hpp"
#include "drm_rows.hpp"

// the error of the calling thread's last refused call, in the signature the .hip units' drm_common.hpp declares (drm_args.hpp)
namespace drm {
int fail(int code, const char *fmt, const char *a = "", long b = 0, long c = 0);
}
#include "drm_args.hpp"
#include "drm_args_whole_body.hpp"
#include "drm_whole_body.hpp"

namespace {
using namespace drm_host;
using drm::fail;

constexpr int64_t CHUNK = 256; // rows per work item (and per partial sum of the backward calls)
thread_local char g_err[512] = "";
std::atomic<int> g_threads{0}; // 0: hardware_concurrency (or DRM_CPU_THREADS)

int64_t n_chunks(int64_t B) { return (B + CHUNK - 1) / CHUNK; }

int pool_size(int64_t chunks) {
    int t = g_threads.load();
    if (t <= 0) {
        const char *e = getenv("DRM_CPU_THREADS");
        t = e ? atoi(e) : (int)std::thread::hardware_concurrency();
    }
    if (t < 1) t = 1;
    if (t > 64) t = 64;
    return (int64_t)t > chunks ? (int)chunks : t;
}

// body(chunk, first_row, rows) for every chunk of B rows, on up to pool_size() threads (the calling thread is one of them)
template <class Body>
void for_chunks(int64_t B, Body body) {
    const int64_t chunks = n_chunks(B);
    if (chunks <= 0) return;
    const int threads = pool_size(chunks);
    std::atomic<int64_t> next{0};
    auto work = [&]() {
        for (;;) {
            const int64_t c = next.fetch_add(1);
            if (c >= chunks) return;
            const int64_t b0 = c * CHUNK;
            body(c, b0, B - b0 < CHUNK ? B - b0 : CHUNK);
        }
    };
    std::vector<std::thread> pool;
    pool.reserve(threads - 1);
    for (int t = 1; t < threads; ++t) pool.emplace_back(work);
    work();
    for (auto &th : pool) th.join();
}

// grad_ops_f = the per-chunk partials added in chunk order (double accumulation)
void reduce_partials(const float *partials, int64_t chunks, int entries, float *out) {
    for (int e = 0; e < entries; ++e) {
        double s = 0.0;
        for (int64_t c = 0; c < chunks; ++c) s += partials[c * entries + e];
        out[e] = (float)s;
    }
}

int fk_any(const drm_walk *w, const float *q, int64_t B, int T, float *pos, float *quat, bool link_major) {
    if (int rc = drm::args_fk(w, q, B, T, pos, quat)) return rc;
    const int n = w->n_dofs;
    for_chunks(B, [&](int64_t, int64_t b0, int64_t rows) {
        if (link_major)
            fk_loop(w, q + b0 * n, rows, T, pos + b0 * 3, quat + b0 * 4, 1, B);
        else
            fk_loop(w, q + b0 * n, rows, T, pos + b0 * T * 3, quat + b0 * T * 4);
    });
    return DRM_OK;
}

int fk_fan(const drm_walk *chains, int T, const float *q, int64_t B, float *pos, float *quat, bool link_major) {
    if (int rc = drm::args_fk_fanout(chains, T, q, B, pos, quat)) return rc;
    const int n = chains[0].n_dofs;
    for_chunks(B, [&](int64_t, int64_t b0, int64_t rows) {
        for (int t = 0; t < T; ++t) {
            if (link_major)
                fk_loop(chains + t, q + b0 * n, rows, 1, pos + (t * B + b0) * 3, quat + (t * B + b0) * 4);
            else
                fk_loop(chains + t, q + b0 * n, rows, 1, pos + (b0 * T + t) * 3, quat + (b0 * T + t) * 4, T, 0);
        }
    });
    return DRM_OK;
}

// drm_operational_space, rows [b0, b0 + rows): jac_loop of the chain, crba_loop and rnea_loop (qdd = 0) of the tree, drm_osc.hpp
template <int M>
void osc_host_rows(const drm_walk *tree, const drm_walk *chain, const float *q, const float *qd, int64_t b0, int64_t rows, int flags,
                   float reg2, float *inertia, float *jbar, float *bias_acc, float *bias_force) {
    const int n = tree->n_dofs;
    const int32_t *w0 = chain->ops_i + DRM_OPI_W0 * chain->capacity;
    std::vector<float> lin(3 * n), ang(3 * n), H((size_t)n * n), nle(n, 0.0f), Xv((size_t)M * n);
    for (int64_t b = b0; b < b0 + rows; ++b) {
        const float *qr = q + b * n, *qdr = qd ? qd + b * n : nullptr;
        bool ok = true;
        for (int k = 0; k < n; ++k) ok = ok && std::isfinite(qr[k]) && (!qdr || std::isfinite(qdr[k]));
        float Lam[M][M], acc[M] = {}, eta[M] = {};
        auto J = [&](int r, int k) -> float { return r < 3 ? lin[r * n + k] : ang[(r - 3) * n + k]; };
        auto X = [&](int r, int k) -> float & { return Xv[(size_t)r * n + k]; };
        if (ok) {
            jac_loop(chain, qr, 1, nullptr, nullptr, lin.data(), ang.data());
            crba_loop(tree, qr, 1, H.data());
            auto Hf = [&](int i, int j) -> float & { return H[(size_t)i * n + j]; };
            drm::osc_ltdl_factor(n, Hf);
            drm::osc_solve_columns<M>(n, Hf, J, X);
            drm::osc_inertia<M>(n, J, X, reg2, Lam);
            if (qdr) {
                drm::osc_bias_acc<M>(chain->n_ops, [&](int k, float *z, float *r, bool &pris, float &v) {
                    const int d = (w0[k] & 0xff) - 1;
                    if (d < 0) return false;
                    pris = (w0[k] >> 26) & 1;
                    const float jp[3] = {lin[d], lin[n + d], lin[2 * n + d]};
                    for (int i = 0; i < 3; ++i) z[i] = pris ? jp[i] : ang[i * n + d];
                    drm::cross3(jp, z, r); // the point of the axis nearest to the target: r = (z x (p - p_k)) x z
                    v = qdr[d];
                    return true;
                }, acc);
                if (bias_force) {
                    rnea_loop(tree, qr, qdr, nullptr, 1, flags & (DRM_RNEA_GRAVITY | DRM_RNEA_DAMPING), nle.data());
                    drm::osc_bias_force<M>(n, X, [&](int k) { return nle[k]; }, acc, Lam, eta);
                }
            }
        }
        for (int i = 0; i < M; ++i) {
            for (int j = 0; j < M; ++j)
                if (inertia) inertia[(b * M + i) * M + j] = ok ? Lam[i][j] : NAN;
            if (bias_acc) bias_acc[b * M + i] = ok ? acc[i] : NAN;
            if (bias_force) bias_force[b * M + i] = ok ? eta[i] : NAN;
        }
        if (jbar)
            for (int k = 0; k < n; ++k)
                for (int c = 0; c < M; ++c) jbar[(b * n + k) * M + c] = ok ? drm::osc_jbar<M>(X, Lam, k, c) : NAN;
    }
}
// drm_forward_dynamics_derivatives, rows [b0, b0 + rows): fd_loop and crba_loop of the row, one reverse sweep of RNEA (rneab_t) per
// row of dID/dq and dID/dqd, then drm_fdd.hpp's inverse and solves
void fdd_host_rows(const drm_walk *w, const float *q, const float *qd, const float *f, int64_t b0, int64_t rows, int flags, float *qdd,
                   float *dq, float *dqd, float *minv) {
    const int n = w->n_dofs;
    std::vector<float> H((size_t)n * n), work(n), acc(n), seed(n), gqdd(n);
    for (int64_t b = b0; b < b0 + rows; ++b) {
        const float *qr = q + b * n, *qdr = qd + b * n, *fr = f + b * n;
        bool ok = true;
        for (int k = 0; k < n; ++k) ok = ok && std::isfinite(qr[k]) && std::isfinite(qdr[k]) && std::isfinite(fr[k]);
        float *Dq = dq + b * n * n, *Dqd = dqd + b * n * n, *Mo = minv + b * n * n;
        if (!ok) {
            for (int k = 0; k < n; ++k) qdd[b * n + k] = NAN;
            for (int k = 0; k < n * n; ++k) Dq[k] = Dqd[k] = Mo[k] = NAN;
            continue;
        }
        fd_loop(w, qr, qdr, fr, 1, flags, acc.data());
        crba_loop(w, qr, 1, H.data());
        for (int k = 0; k < n; ++k) { // row k of dID/dq and dID/dqd, in place in the outputs
            for (int d = 0; d < n; ++d) seed[d] = d == k ? 1.0f : 0.0f;
            rneab_t(w, qr, qdr, acc.data(), 1, flags, seed.data(), 0, Dq + k * n, Dqd + k * n, gqdd.data(), nullptr);
        }
        auto Hf = [&](int i, int j) -> float & { return H[(size_t)i * n + j]; };
        auto wf = [&](int i) -> float & { return work[i]; };
        drm::fdd_ltdl_factor<float>(n, Hf);
        drm::fdd_inverse<float>(n, Hf, wf, [&](int i, int c, float v) { Mo[i * n + c] = v; Mo[c * n + i] = v; });
        drm::fdd_solve_columns<float>(n, Hf, wf, [&](int i, int j) { return Dq[i * n + j]; }, [&](int i, int j, float v) { Dq[i * n + j] = v; });
        drm::fdd_solve_columns<float>(n, Hf, wf, [&](int i, int j) { return Dqd[i * n + j]; }, [&](int i, int j, float v) { Dqd[i * n + j] = v; });
        for (int k = 0; k < n; ++k) qdd[b * n + k] = acc[k];
    }
}
// drm_rnea_regressor, rows [b0, b0 + rows): drm_regressor.hpp's walk of the row, its records on this thread's heap
void regressor_host_rows(const drm_walk *w, const float *q, const float *qd, const float *qdd, int64_t b0, int64_t rows, int flags, float *Y) {
    const int n = w->n_dofs, n_ops = w->n_ops;
    const bool damping = (flags & DRM_RNEA_DAMPING) != 0;
    const int64_t P = (int64_t)drm::REG_COLS * n_ops + (damping ? n : 0);
    const Ctl ctl(w);
    std::vector<float> rec((size_t)3 * (n_ops > 0 ? n_ops : 1));
    Motion ms[DRM_MAX_SLOTS];
    for (int64_t b = b0; b < b0 + rows; ++b) {
        const float *qr = q + b * n, *qdr = qd + b * n, *qddr = qdd ? qdd + b * n : nullptr;
        float *Yr = Y + b * n * P;
        for (int64_t i = 0; i < n * P; ++i) Yr[i] = 0.0f;
        drm::regressor_tree_walk(
            n_ops, w->n_segments > 1 ? w->prefix_end : 0, ctl, [&](int k) { return w->ops_f + k * DRM_OPF_STRIDE; },
            (flags & DRM_RNEA_GRAVITY) ? 9.81f : 0.0f, [&](int d, float &a, float &v, float &acc) { a = qr[d]; v = qdr[d]; acc = qddr ? qddr[d] : 0.0f; },
            [&](int k, float c, float s, float x) { rec[3 * k] = c; rec[3 * k + 1] = s; rec[3 * k + 2] = x; },
            [&](int k, float &c, float &s, float &x) { c = rec[3 * k]; s = rec[3 * k + 1]; x = rec[3 * k + 2]; },
            [&](int sl, const Motion &M) { ms[sl] = M; }, [&](int sl, Motion &M) { M = ms[sl]; },
            [&](int dof, int op, int col, float v) { Yr[dof * P + drm::REG_COLS * op + col] = v; });
        if (damping)
            for (int j = 0; j < n; ++j) Yr[j * P + drm::REG_COLS * n_ops + j] = qdr[j];
    }
}
// one row's `count` records of N floats on this thread's heap, in the put / get shape of the rows kernels' lane view (drm_rows.hpp)
template <int N>
struct HostRecords : drm::Records<N, 1> {
    std::vector<float> mem;
    explicit HostRecords(int count) : mem((size_t)N * (count > 0 ? count : 1)) { this->base = mem.data(); }
};
// drm_lagrangian_dynamics, rows [b0, b0 + rows): drm_lagrangian.hpp's walk of the row, its records on this thread's heap
void lagrangian_host_rows(const drm_walk *w, const float *q, const float *qd, int64_t b0, int64_t rows, float *H, float *C, float *g) {
    const int n = w->n_dofs, n_ops = w->n_ops, n_slots = w->n_slots;
    const Ctl ctl(w);
    HostRecords<drm::LAG_REC_FLOATS> rec(n_ops); HostRecords<drm::LAG_SLOT_FLOATS> slots(n_slots);
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (int64_t b = b0; b < b0 + rows; ++b) {
        const float *qr = q + b * n, *qdr = qd + b * n;
        float *Hr = H ? H + b * n * n : nullptr, *Cr = C ? C + b * n * n : nullptr, *gr = g ? g + b * n : nullptr;
        bool bad = false;
        for (int d = 0; d < n; ++d) bad = bad || drm::lag_bad_input(qr[d], qdr[d]);
        for (int64_t i = 0; i < n * n; ++i) {
            if (Hr) Hr[i] = 0.0f;
            if (Cr) Cr[i] = 0.0f;
        }
        drm::lagrangian_tree_walk(
            n_ops, w->n_segments > 1 ? w->prefix_end : 0, n_slots, ctl, [&](int k) { return w->ops_f + k * DRM_OPF_STRIDE; },
            [&](int d, float &a, float &v) { a = bad ? 0.0f : qr[d]; v = bad ? 0.0f : qdr[d]; },
            [&](int k, const float *x) { rec.put(k, x); }, [&](int k, float *x) { rec.get(k, x); },
            [&](int s, const float *x) { slots.put(s, x); }, [&](int s, float *x) { slots.get(s, x); },
            [&](int i, int j, float v) { if (Hr) Hr[i * n + j] = bad ? nan : v; },
            [&](int i, int j, float v) { if (Cr) Cr[i * n + j] = bad ? nan : v; },
            [&](int j, float v) { if (gr) gr[j] = bad ? nan : v; });
    }
}
// drm_rnea_derivatives, rows [b0, b0 + rows): drm_idd.hpp's walk of the row, its records on this thread's heap
void idd_host_rows(const drm_walk *w, const float *q, const float *qd, const float *qdd, int64_t b0, int64_t rows, int flags, float *tau,
                   float *dq, float *dqd, float *H) {
    const int n = w->n_dofs, n_ops = w->n_ops, n_slots = w->n_slots;
    const Ctl ctl(w);
    HostRecords<drm::IDD_REC_FLOATS> rec(n_ops); HostRecords<drm::IDD_SLOT_FLOATS> slots(n_slots);
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (int64_t b = b0; b < b0 + rows; ++b) {
        const float *qr = q + b * n, *qdr = qd + b * n, *qddr = qdd + b * n;
        float *tr = tau ? tau + b * n : nullptr;
        float *Mr[3] = {dq ? dq + b * n * n : nullptr, dqd ? dqd + b * n * n : nullptr, H ? H + b * n * n : nullptr};
        bool bad = false;
        for (int d = 0; d < n; ++d) bad = bad || drm::idd_bad_input(qr[d], qdr[d], qddr[d]);
        for (float *M : Mr)
            if (M) std::fill(M, M + (size_t)n * n, 0.0f);
        drm::idd_tree_walk(
            n_ops, w->n_segments > 1 ? w->prefix_end : 0, n_slots, (flags & DRM_RNEA_GRAVITY) ? 9.81f : 0.0f, (flags & DRM_RNEA_DAMPING) != 0, ctl,
            [&](int k) { return w->ops_f + k * DRM_OPF_STRIDE; },
            [&](int d, float &a, float &v, float &acc) { a = bad ? 0.0f : qr[d]; v = bad ? 0.0f : qdr[d]; acc = bad ? 0.0f : qddr[d]; },
            [&](int k, const float *x) { rec.put(k, x); }, [&](int k, float *x) { rec.get(k, x); },
            [&](int s, const float *x) { slots.put(s, x); }, [&](int s, float *x) { slots.get(s, x); },
            [&](int which, int i, int j, float v) { if (Mr[which]) Mr[which][i * n + j] = bad ? nan : v; },
            [&](int j, float v) { if (tr) tr[j] = bad ? nan : v; });
    }
}
// drm_energy, rows [b0, b0 + rows): drm_energy.hpp's walk of the row, its records on this thread's heap
void energy_host_rows(const drm_walk *w, const float *q, const float *qd, int64_t b0, int64_t rows, float *T, float *V, float *p, float *dT,
                      float *g) {
    const int n = w->n_dofs, n_ops = w->n_ops, n_slots = w->n_slots;
    const Ctl ctl(w);
    HostRecords<drm::ENERGY_REC_FLOATS> rec(n_ops); HostRecords<drm::ENERGY_SLOT_FLOATS> slots(n_slots);
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (int64_t b = b0; b < b0 + rows; ++b) {
        const float *qr = q + b * n, *qdr = qd + b * n;
        float *pr = p ? p + b * n : nullptr, *dr = dT ? dT + b * n : nullptr, *gr = g ? g + b * n : nullptr;
        bool bad = false;
        for (int d = 0; d < n; ++d) bad = bad || drm::lag_bad_input(qr[d], qdr[d]);
        drm::energy_tree_walk(
            n_ops, w->n_segments > 1 ? w->prefix_end : 0, n_slots, p || dT || g, ctl, [&](int k) { return w->ops_f + k * DRM_OPF_STRIDE; },
            [&](int d, float &a, float &v) { a = bad ? 0.0f : qr[d]; v = bad ? 0.0f : qdr[d]; },
            [&](int k, const float *x) { rec.put(k, x); }, [&](int k, float *x) { rec.get(k, x); },
            [&](int s, const float *x) { slots.put(s, x); }, [&](int s, float *x) { slots.get(s, x); },
            [&](float Tv, float Vv) {
                if (T) T[b] = bad ? nan : Tv;
                if (V) V[b] = bad ? nan : Vv;
            },
            [&](int j, float pj, float dj, float gj) {
                if (j >= n) return;
                if (pr) pr[j] = bad ? nan : pj;
                if (dr) dr[j] = bad ? nan : dj;
                if (gr) gr[j] = bad ? nan : gj;
            });
    }
}
// the walks drm_links.hip's fused kernels take: a serial 7-DoF arm chain of 8 ops, every op a target in walk order.  The host build
// runs their straight-line arithmetic (drm_links.hpp link_chain_*) on every row of such a call, the general walk with DRM_LINKS_COMPOSED.
bool links_chain_walk(const drm_walk *w, int T, int flags) {
    return !(flags & DRM_LINKS_COMPOSED) && (w->shape & DRM_WALK_ARM_CHAIN) && (w->shape & DRM_WALK_TARGETS_ORDERED) && w->capacity == 8 &&
           w->n_dofs == 7 && w->n_ops == 8 && T == 8;
}
// drm_link_motion, rows [b0, b0 + rows)
template <int MODE>
void link_motion_host_rows(const drm_walk *w, const float *q, const float *qd, const float *qdd, int64_t b0, int64_t rows, int T, int flags,
                           float *pos, float *lv, float *av, float *la, float *aa) {
    const int n = w->n_dofs, n_ops = w->n_ops, n_slots = w->n_slots;
    const Ctl ctl(w);
    HostRecords<drm::LINKS_SLOT_FLOATS> slots(n_slots);
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const bool chain = links_chain_walk(w, T, flags);
    auto row = [&](int k) { return w->ops_f + k * DRM_OPF_STRIDE; };
    for (int64_t b = b0; b < b0 + rows; ++b) {
        const float *qr = q + b * n, *qdr = (MODE >= 1 && qd) ? qd + b * n : nullptr, *qddr = (MODE >= 2 && qdd) ? qdd + b * n : nullptr;
        bool bad = false;
        for (int d = 0; d < n; ++d) bad = bad || drm::links_bad_input(qr[d], qdr ? qdr[d] : 0.0f, qddr ? qddr[d] : 0.0f);
        auto emit = [&](int t, const drm::LinkState &st) {
            if (t >= T) return;
            const int64_t at = (b * T + t) * 3;
            for (int i = 0; i < 3; ++i) {
                if (pos) pos[at + i] = bad ? nan : st.p[i];
                if (MODE >= 1 && lv) lv[at + i] = bad ? nan : st.v[i];
                if (MODE >= 1 && av) av[at + i] = bad ? nan : st.w[i];
                if (MODE >= 2 && la) la[at + i] = bad ? nan : st.a[i];
                if (MODE >= 2 && aa) aa[at + i] = bad ? nan : st.al[i];
            }
        };
        if (chain) {
            float qv[7], qdv[7], qddv[7], cs[7], sn[7];
            for (int d = 0; d < 7; ++d) {
                qv[d] = bad ? 0.0f : qr[d];
                qdv[d] = (bad || !qdr) ? 0.0f : qdr[d];
                qddv[d] = (bad || !qddr) ? 0.0f : qddr[d];
            }
            drm::chain_trig<7>(qv, cs, sn);
            drm::link_chain_motion<8, 7, (MODE >= 1), (MODE >= 2)>(row, cs, sn, qdv, qddv, emit);
            continue;
        }
        drm::link_motion_walk<(MODE >= 1), (MODE >= 2)>(
            n_ops, n_slots, ctl, row,
            [&](int d, float &a, float &v, float &acc) {
                a = bad ? 0.0f : qr[d];
                v = (bad || !qdr) ? 0.0f : qdr[d];
                acc = (bad || !qddr) ? 0.0f : qddr[d];
            },
            [&](int s, const float *x) { slots.put(s, x); }, [&](int s, float *x) { slots.get(s, x); }, emit);
    }
}
// drm_external_torques, rows [b0, b0 + rows)
void link_torques_host_rows(const drm_walk *w, const float *q, const float *force, const float *torque, int64_t b0, int64_t rows, int T,
                            int flags, float *tau) {
    const int n = w->n_dofs, n_ops = w->n_ops, n_slots = w->n_slots;
    const Ctl ctl(w);
    HostRecords<drm::LINKS_REC_FLOATS> rec(n_ops); HostRecords<drm::LINKS_SLOT_FLOATS> slots(n_slots);
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const bool chain = links_chain_walk(w, T, flags);
    auto row = [&](int k) { return w->ops_f + k * DRM_OPF_STRIDE; };
    for (int64_t b = b0; b < b0 + rows; ++b) {
        const float *qr = q + b * n, *fr = force ? force + b * T * 3 : nullptr, *mr = torque ? torque + b * T * 3 : nullptr;
        float *tr = tau + b * n;
        bool bad = false;
        for (int d = 0; d < n; ++d) bad = bad || drm::lag_bad_input(qr[d], 0.0f);
        for (int d = 0; d < n; ++d) tr[d] = bad ? nan : 0.0f;
        auto wrench = [&](int t, float *f, float *m) {
            for (int i = 0; i < 3; ++i) {
                f[i] = (fr && t < T) ? fr[3 * t + i] : 0.0f;
                m[i] = (mr && t < T) ? mr[3 * t + i] : 0.0f;
            }
        };
        auto jout = [&](int j, float v) { if (j < n) tr[j] = bad ? nan : v; };
        if (chain) {
            float qv[7], cs[7], sn[7];
            for (int d = 0; d < 7; ++d) qv[d] = bad ? 0.0f : qr[d];
            drm::chain_trig<7>(qv, cs, sn);
            drm::link_chain_torques<8, 7>(row, cs, sn, wrench, jout);
            continue;
        }
        drm::link_torques_walk(
            n_ops, n_slots, ctl, row, [&](int d) { return bad ? 0.0f : qr[d]; },
            [&](int k, const float *x) { rec.put(k, x); }, [&](int k, float *x) { rec.get(k, x); },
            [&](int s, const float *x) { slots.put(s, x); }, [&](int s, float *x) { slots.get(s, x); }, wrench, jout);
    }
}
// drm_link_power_dq, rows [b0, b0 + rows)
void link_power_dq_host_rows(const drm_walk *w, const float *q, const float *qd, const float *force, const float *torque, int64_t b0,
                             int64_t rows, int T, int flags, float *dq, float *tau) {
    const int n = w->n_dofs, n_ops = w->n_ops, n_slots = w->n_slots;
    const Ctl ctl(w);
    HostRecords<drm::LINKS_DQ_REC_FLOATS> rec(n_ops); HostRecords<drm::LINKS_SLOT_FLOATS> slots(n_slots);
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const bool chain = links_chain_walk(w, T, flags);
    auto row = [&](int k) { return w->ops_f + k * DRM_OPF_STRIDE; };
    for (int64_t b = b0; b < b0 + rows; ++b) {
        const float *qr = q + b * n, *qdr = qd + b * n;
        const float *fr = force ? force + b * T * 3 : nullptr, *mr = torque ? torque + b * T * 3 : nullptr;
        float *gr = dq + b * n, *tr = tau ? tau + b * n : nullptr;
        bool bad = false;
        for (int d = 0; d < n; ++d) bad = bad || drm::lag_bad_input(qr[d], qdr[d]);
        for (int d = 0; d < n; ++d) {
            gr[d] = bad ? nan : 0.0f;
            if (tr) tr[d] = bad ? nan : 0.0f;
        }
        auto wrench = [&](int t, float *f, float *m) {
            for (int i = 0; i < 3; ++i) {
                f[i] = (fr && t < T) ? fr[3 * t + i] : 0.0f;
                m[i] = (mr && t < T) ? mr[3 * t + i] : 0.0f;
            }
        };
        auto jout = [&](int j, float g, float t) {
            if (j >= n) return;
            gr[j] = bad ? nan : g;
            if (tr) tr[j] = bad ? nan : t;
        };
        if (chain) {
            float qv[7], qdv[7], cs[7], sn[7];
            for (int d = 0; d < 7; ++d) { qv[d] = bad ? 0.0f : qr[d]; qdv[d] = bad ? 0.0f : qdr[d]; }
            drm::chain_trig<7>(qv, cs, sn);
            drm::link_chain_power_dq<8, 7>(row, cs, sn, qdv, wrench, jout);
            continue;
        }
        drm::link_power_dq_walk(
            n_ops, n_slots, ctl, row, [&](int d, float &a, float &v) { a = bad ? 0.0f : qr[d]; v = bad ? 0.0f : qdr[d]; },
            [&](int k, const float *x) { rec.put(k, x); }, [&](int k, float *x) { rec.get(k, x); },
            [&](int s, const float *x) { slots.put(s, x); }, [&](int s, float *x) { slots.get(s, x); }, wrench, jout);
    }
}
using drm::ContactPlan;
// out = tau_in + (tau_ext + tau_lim) of `rows` rows from q, qd on (all pointers at the first of them; tau_in, force, moment may be
// NULL): the chain form where drm_contact.hip would launch its fused kernels, elsewhere its composition of the link sweeps and the law.
// check_rows: a row whose q or qd cannot be used gets NaN (drm_contact_torques).
void contact_host_rows(const drm_walk *lw, const ContactPlan &a, const float *q, const float *qd, const float *tau_in, int64_t rows, int T,
                       int n, int flags, bool check_rows, float *out, float *force, float *moment) {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    std::vector<float> ext((size_t)rows * n, 0.0f);
    if (a.has_plane && links_chain_walk(lw, T, flags)) {
        auto row = [&](int k) { return lw->ops_f + k * DRM_OPF_STRIDE; };
        for (int64_t b = 0; b < rows; ++b) {
            bool bad = false;
            for (int d = 0; d < 7; ++d) bad = bad || drm::lag_bad_input(q[b * 7 + d], qd[b * 7 + d]);
            float qv[7], qdv[7], cs[7], sn[7];
            for (int d = 0; d < 7; ++d) { qv[d] = bad ? 0.0f : q[b * 7 + d]; qdv[d] = bad ? 0.0f : qd[b * 7 + d]; }
            drm::chain_trig<7>(qv, cs, sn);
            drm::contact_chain_torques<8, 7>(
                row, a.pl, cs, sn, qdv, [&](int k) { return a.radius ? a.radius[k] : 0.0f; },
                [&](int k, const float *f, const float *m) {
                    for (int i = 0; i < 3; ++i) {
                        if (force) force[(b * 8 + k) * 3 + i] = bad ? nan : f[i];
                        if (moment) moment[(b * 8 + k) * 3 + i] = bad ? nan : m[i];
                    }
                },
                [&](int j, float v) { ext[b * 7 + j] = v; });
        }
    } else if (a.has_plane) {
        const size_t L = (size_t)rows * T * 3;
        std::vector<float> pos(L), lv(L), av(L), fbuf(force ? 0 : L), mbuf(moment ? 0 : L);
        float *f = force ? force : fbuf.data(), *m = moment ? moment : mbuf.data();
        link_motion_host_rows<1>(lw, q, qd, nullptr, 0, rows, T, flags, pos.data(), lv.data(), av.data(), nullptr, nullptr);
        for (int64_t i = 0; i < rows * T; ++i) {
            float fi[3], mi[3];
            drm::contact_wrench(a.pl, a.radius ? a.radius[i % T] : 0.0f, &pos[3 * i], &lv[3 * i], &av[3 * i], fi, mi);
            const bool bad = pos[3 * i] != pos[3 * i];
            for (int k = 0; k < 3; ++k) { f[3 * i + k] = bad ? nan : fi[k]; m[3 * i + k] = bad ? nan : mi[k]; }
        }
        link_torques_host_rows(lw, q, f, m, 0, rows, T, flags, ext.data());
    }
    for (int64_t b = 0; b < rows; ++b) {
        bool bad = false;
        if (check_rows)
            for (int d = 0; d < n; ++d) bad = bad || drm::lag_bad_input(q[b * n + d], qd[b * n + d]);
        for (int d = 0; d < n; ++d) {
            const int64_t i = b * n + d;
            float e = ext[i];
            if (a.lower) e += drm::joint_spring_torque(a.k, a.c, a.lower[d], a.upper[d], q[i], qd[i]);
            if (bad) e = nan;
            out[i] = tau_in ? tau_in[i] + e : e;
        }
    }
}
// drm_contact_torques_vjp of `rows` rows from q, qd, lam on (grad_q or grad_qd may be NULL): the chain form where drm_contact.hip would
// launch its fused kernel, elsewhere its composition of the link sweeps, the law's backward and the q-gradients of the sweeps.
void contact_vjp_host_rows(const drm_walk *lw, const ContactPlan &a, const float *q, const float *qd, const float *lam, int64_t rows, int T,
                           int n, int flags, float *grad_q, float *grad_qd) {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const size_t N = (size_t)rows * n;
    std::vector<float> gq(N, 0.0f), gqd(N, 0.0f);
    auto row_bad = [&](int64_t b) {
        bool bad = false;
        for (int d = 0; d < n; ++d) bad = bad || drm::lag_bad_input(q[b * n + d], qd[b * n + d]) || !(std::fabs(lam[b * n + d]) <= 3.0e38f);
        return bad;
    };
    if (a.has_plane && links_chain_walk(lw, T, flags)) {
        auto row = [&](int k) { return lw->ops_f + k * DRM_OPF_STRIDE; };
        for (int64_t b = 0; b < rows; ++b) {
            const bool bad = row_bad(b);
            float qv[7], qdv[7], lv[7], cs[7], sn[7];
            for (int d = 0; d < 7; ++d) {
                qv[d] = bad ? 0.0f : q[b * 7 + d]; qdv[d] = bad ? 0.0f : qd[b * 7 + d]; lv[d] = bad ? 0.0f : lam[b * 7 + d];
            }
            drm::chain_trig<7>(qv, cs, sn);
            drm::contact_chain_torques_vjp<8, 7>(
                row, a.pl, cs, sn, qdv, lv, [&](int k) { return a.radius ? a.radius[k] : 0.0f; },
                [&](int j, float x, float y) { gq[b * 7 + j] = x; gqd[b * 7 + j] = y; });
        }
    } else if (a.has_plane) {
        const size_t L = (size_t)rows * T * 3;
        std::vector<float> pos(L), lv(L), av(L), la(L), lb(L), f(L), m(L), gp(L), gv(L), gw(L), o1(N), o2(N), o3(N);
        link_motion_host_rows<1>(lw, q, qd, nullptr, 0, rows, T, flags, pos.data(), lv.data(), av.data(), nullptr, nullptr);
        link_motion_host_rows<1>(lw, q, lam, nullptr, 0, rows, T, flags, nullptr, la.data(), lb.data(), nullptr, nullptr);
        for (int64_t i = 0; i < rows * T; ++i)
            drm::contact_wrench_vjp(a.pl, a.radius ? a.radius[i % T] : 0.0f, &pos[3 * i], &lv[3 * i], &av[3 * i], &la[3 * i], &lb[3 * i],
                                    &f[3 * i], &m[3 * i], &gp[3 * i], &gv[3 * i], &gw[3 * i]);
        link_power_dq_host_rows(lw, q, lam, f.data(), m.data(), 0, rows, T, flags, o1.data(), nullptr);
        link_torques_host_rows(lw, q, gp.data(), nullptr, 0, rows, T, flags, o2.data());
        link_power_dq_host_rows(lw, q, qd, gv.data(), gw.data(), 0, rows, T, flags, o3.data(), gqd.data());
        for (size_t i = 0; i < N; ++i) gq[i] = (o1[i] + o2[i]) + o3[i];
    }
    for (int64_t b = 0; b < rows; ++b) {
        const bool bad = row_bad(b);
        for (int d = 0; d < n; ++d) {
            const int64_t i = b * n + d;
            float x = gq[i], y = gqd[i];
            if (a.lower) drm::joint_spring_vjp(a.k, a.c, a.lower[d], a.upper[d], q[i], lam[i], x, y);
            if (grad_q) grad_q[i] = bad ? nan : x;
            if (grad_qd) grad_qd[i] = bad ? nan : y;
        }
    }
}
// drm_collision_cost (cost, dq) / drm_sphere_distances (center, wd, sd) of `rows` rows (all pointers at the first of them, any may be
// NULL): the targets' frames by the chain form where drm_collision.hip would launch its fused kernel, by the general walk elsewhere;
// the law per row (drm_collision.hpp coll_row); dq by link_torques_host_rows.
void collision_host_rows(const drm_walk *w, const drm::CollTables &t, const float *q, int64_t rows, int flags, float *cost, float *dq,
                         float *center, float *wd, float *sd) {
    const int n = w->n_dofs, T = t.T, S = t.S;
    const Ctl ctl(w);
    HostRecords<drm::LINKS_SLOT_FLOATS> slots(w->n_slots);
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const bool chain = links_chain_walk(w, T, flags) && drm::coll_within_caps(S, t.n_ws + t.n_wb, t.P);
    std::vector<float> R((size_t)9 * T), p((size_t)3 * T), cen(center ? 0 : (size_t)3 * S);
    std::vector<float> F(dq ? (size_t)rows * T * 3 : 0), M(F.size());
    auto row = [&](int k) { return w->ops_f + k * DRM_OPF_STRIDE; };
    for (int64_t b = 0; b < rows; ++b) {
        const float *qr = q + b * n;
        bool bad = false;
        for (int d = 0; d < n; ++d) bad = bad || drm::lag_bad_input(qr[d], 0.0f);
        auto emit = [&](int k, const drm::LinkState &st) {
            if (k >= T) return;
            for (int i = 0; i < 9; ++i) R[9 * k + i] = st.R[i];
            for (int i = 0; i < 3; ++i) p[3 * k + i] = st.p[i];
        };
        if (chain) {
            float qv[7], cs[7], sn[7];
            const float zero[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            for (int d = 0; d < 7; ++d) qv[d] = bad ? 0.0f : qr[d];
            drm::chain_trig<7>(qv, cs, sn);
            drm::link_chain_motion<8, 7, false, false>(row, cs, sn, zero, zero, emit);
        } else {
            drm::link_motion_walk<false, false>(
                w->n_ops, w->n_slots, ctl, row,
                [&](int d, float &x, float &v, float &acc) { x = bad ? 0.0f : qr[d]; v = 0.0f; acc = 0.0f; },
                [&](int s, const float *x) { slots.put(s, x); }, [&](int s, float *x) { slots.get(s, x); }, emit);
        }
        float *cr = center ? center + b * S * 3 : cen.data();
        const float c = drm::coll_row(t, R.data(), p.data(), cr, dq ? &F[(size_t)b * T * 3] : nullptr, dq ? &M[(size_t)b * T * 3] : nullptr,
                                      wd ? wd + b * S : nullptr, sd ? sd + b * S : nullptr);
        if (cost) cost[b] = bad ? nan : c;
        if (bad)
            for (int s = 0; s < S; ++s) {
                if (center) cr[3 * s] = cr[3 * s + 1] = cr[3 * s + 2] = nan;
                if (wd) wd[b * S + s] = nan;
                if (sd) sd[b * S + s] = nan;
            }
    }
    if (dq) link_torques_host_rows(w, q, F.data(), M.data(), 0, rows, T, flags, dq);
}
} // namespace

int drm::fail(int code, const char *fmt, const char *a, long b, long c) {
    snprintf(g_err, sizeof(g_err), fmt, a, b, c);
    return code;
}

extern "C" {
int drm_abi_version(void) { return DRM_ABI_VERSION; }
int drm_walk_sizeof(void) { return (int)sizeof(drm_walk); }
const char *drm_last_error(void) { return g_err; }
// libdrm_cpu.so only: the number of threads the calls may use (0 = all cores / DRM_CPU_THREADS)
void drm_cpu_set_threads(int n) { g_threads.store(n); }
int drm_special_load(const char *, const char *, const void **) {
    return fail(DRM_ERR_UNSUPPORTED, "per-robot code objects are HIP kernels: not available in the host build");
}

int drm_fk(const drm_walk *w, const float *q, int64_t B, int32_t T, float *pos, float *quat, void *) {
    return fk_any(w, q, B, T, pos, quat, false);
}
int drm_fk_links(const drm_walk *w, const float *q, int64_t B, int32_t T, float *pos, float *quat, void *) {
    return fk_any(w, q, B, T, pos, quat, true);
}
int drm_fk_fanout(const drm_walk *chains, int32_t T, const float *q, int64_t B, float *pos, float *quat, void *) {
    return fk_fan(chains, T, q, B, pos, quat, false);
}
int drm_fk_fanout_links(const drm_walk *chains, int32_t T, const float *q, int64_t B, float *pos, float *quat, void *) {
    return fk_fan(chains, T, q, B, pos, quat, true);
}

int drm_fk_jacobian(const drm_walk *w, const float *q, int64_t B, float *pos, float *quat, float *lin, float *ang, void *) {
    if (int rc = drm::args_fk_jacobian(w, q, B, lin, ang)) return rc;
    const int n = w->n_dofs;
    for_chunks(B, [&](int64_t, int64_t b0, int64_t rows) {
        jac_loop(w, q + b0 * n, rows, pos ? pos + b0 * 3 : nullptr, quat ? quat + b0 * 4 : nullptr, lin + b0 * 3 * n, ang + b0 * 3 * n);
    });
    return DRM_OK;
}

// no scratch anywhere in the host build: every thread keeps its per-link records on its own stack / heap
int64_t drm_rnea_scratch_floats(const drm_walk *, int64_t) { return 0; }
int64_t drm_rnea_scratch_floats_aligned(const drm_walk *, int64_t) { return 0; }
int64_t drm_crba_scratch_floats(const drm_walk *, int64_t) { return 0; }
int64_t drm_crba_scratch_floats_aligned(const drm_walk *, int64_t) { return 0; }
int64_t drm_forward_dynamics_scratch_floats(const drm_walk *, int64_t) { return 0; }
int64_t drm_forward_dynamics_scratch_floats_aligned(const drm_walk *, int64_t) { return 0; }

int drm_rnea(const drm_walk *w, const float *q, const float *qd, const float *qdd, int64_t B, int32_t flags, float *tau, float *,
             void *) {
    if (int rc = drm::args_rnea(w, q, qd, B, tau)) return rc;
    const int n = w->n_dofs;
    for_chunks(B, [&](int64_t, int64_t b0, int64_t rows) {
        rnea_loop(w, q + b0 * n, qd + b0 * n, qdd ? qdd + b0 * n : nullptr, rows, flags, tau + b0 * n);
    });
    return DRM_OK;
}

int drm_fk_rnea(const drm_walk *tree, const drm_walk *chain, int32_t, const float *q, const float *qd, const float *qdd, int64_t B,
                int32_t flags, float *tau, float *pos, float *quat, float *, void *) {
    if (int rc = drm::args_fk_rnea(tree, chain, q, qd, B, tau, pos, quat)) return rc;
    const int n = tree->n_dofs;
    for_chunks(B, [&](int64_t, int64_t b0, int64_t rows) {
        rnea_loop(tree, q + b0 * n, qd + b0 * n, qdd ? qdd + b0 * n : nullptr, rows, flags, tau + b0 * n);
        fk_loop(chain, q + b0 * n, rows, 1, pos + b0 * 3, quat + b0 * 4);
    });
    return DRM_OK;
}

// ABI 11: the host build of the one-sided gather — the destinations are host arrays (e.g. shared-memory tensors of the other ranks)
int drm_fk_rnea_put(const drm_walk *tree, const drm_walk *chain, int32_t target_op, const float *q, const float *qd, const float *qdd,
                    int64_t B, int32_t flags, float *tau, float *pos, float *quat, float *scratch, const drm_put *put, void *stream) {
    if (int rc = drm::args_fk_rnea_put(tree, chain, q, qd, B, tau, pos, quat, put)) return rc;
    if (int rc = drm_fk_rnea(tree, chain, target_op, q, qd, qdd, B, flags, tau, pos, quat, scratch, stream)) return rc;
    if (!put || B == 0) return DRM_OK;
    const int n = tree->n_dofs;
    for (int p = 0; p < put->n_peers; ++p) {
        if (put->tau[p]) memcpy(put->tau[p] + put->row_offset * n, tau, sizeof(float) * (size_t)B * n);
        if (put->pos[p]) memcpy(put->pos[p] + put->row_offset * 3, pos, sizeof(float) * (size_t)B * 3);
        if (put->quat[p]) memcpy(put->quat[p] + put->row_offset * 4, quat, sizeof(float) * (size_t)B * 4);
    }
    return DRM_OK;
}

int drm_crba(const drm_walk *w, const float *q, int64_t B, float *H, float *, void *) {
    if (int rc = drm::args_crba(w, q, B, H)) return rc;
    const int n = w->n_dofs;
    for_chunks(B, [&](int64_t, int64_t b0, int64_t rows) { crba_loop(w, q + b0 * n, rows, H + b0 * n * n); });
    return DRM_OK;
}

int drm_forward_dynamics(const drm_walk *w, const float *q, const float *qd, const float *f, int64_t B, int32_t flags, float *qdd,
                         float *, void *) {
    if (int rc = drm::args_forward_dynamics(w, q, qd, f, B, qdd)) return rc;
    const int n = w->n_dofs;
    for_chunks(B, [&](int64_t, int64_t b0, int64_t rows) {
        fd_loop(w, q + b0 * n, qd + b0 * n, f + b0 * n, rows, flags, qdd + b0 * n);
    });
    return DRM_OK;
}

// ABI 14: every chunk of rows runs its T steps on its own (fd_loop, then the integrator of drm_rollout.hpp), the state of step t read
// back from the slab step t - 1 wrote
int64_t drm_forward_dynamics_rollout_scratch_floats(const drm_walk *, int64_t) { return 0; }
int64_t drm_forward_dynamics_rollout_scratch_floats_aligned(const drm_walk *, int64_t) { return 0; }

int drm_forward_dynamics_rollout(const drm_walk *w, const float *q0, const float *qd0, const float *tau, int64_t B, int32_t T, float dt,
                                 int32_t flags, float *q_traj, float *qd_traj, float *qdd_traj, float *, void *) {
    if (int rc = drm::args_forward_dynamics_rollout(w, q0, qd0, tau, B, T, dt, q_traj, qd_traj)) return rc;
    const int n = w->n_dofs, fd_flags = flags & (DRM_RNEA_GRAVITY | DRM_RNEA_DAMPING);
    const bool expl = (flags & DRM_ROLLOUT_EXPLICIT_EULER) != 0;
    const int64_t slab = B * n;
    for_chunks(B, [&](int64_t, int64_t b0, int64_t rows) {
        std::vector<float> acc(qdd_traj ? 0 : (size_t)rows * n);
        for (int t = 0; t < T; ++t) {
            const int64_t off = (int64_t)t * slab + b0 * n;
            const float *qi = t ? q_traj + off - slab : q0 + b0 * n, *qdi = t ? qd_traj + off - slab : qd0 + b0 * n;
            float *a = qdd_traj ? qdd_traj + off : acc.data();
            fd_loop(w, qi, qdi, tau + off, rows, fd_flags, a);
            for (int64_t i = 0; i < rows * n; ++i) {
                float x = qi[i], v = qdi[i];
                drm::rollout_step(x, v, a[i], dt, expl);
                q_traj[off + i] = x;
                qd_traj[off + i] = v;
            }
        }
    });
    return DRM_OK;
}

// ABI 15: every row runs its iterations on its own: jac_loop of the row, then drm_ik.hpp's update, until it stops
int64_t drm_inverse_kinematics_scratch_floats(const drm_walk *, int64_t) { return 0; }
int64_t drm_inverse_kinematics_scratch_floats_aligned(const drm_walk *, int64_t) { return 0; }

int drm_inverse_kinematics(const drm_walk *w, const float *q0, const float *target_pos, const float *target_quat, int64_t B,
                           int32_t max_iters, float damping, float step, float tol_pos, float tol_rot, const float *lower,
                           const float *upper, int32_t flags, float *q, float *err, int32_t *iters, float *, void *) {
    if (int rc = drm::args_inverse_kinematics(w, q0, target_pos, target_quat, B, max_iters, damping, step, tol_pos, tol_rot, lower, upper, flags, q, err))
        return rc;
    const bool pos_only = (flags & DRM_IK_POSITION_ONLY) != 0;
    const int n = w->n_dofs;
    const drm::IkOpts o = {damping * damping, step, tol_pos, tol_rot};
    for_chunks(B, [&](int64_t, int64_t b0, int64_t rows) {
        std::vector<float> lin(3 * n), ang(3 * n);
        for (int64_t b = b0; b < b0 + rows; ++b) {
            float *qr = q + b * n;
            for (int k = 0; k < n; ++k) qr[k] = q0[b * n + k];
            float tq[4] = {0.0f, 0.0f, 0.0f, 1.0f};
            if (!pos_only) {
                for (int k = 0; k < 4; ++k) tq[k] = target_quat[b * 4 + k];
                drm::ik_normalize_quat(tq);
            }
            auto J = [&](int r, int k) -> float { return r < 3 ? lin[r * n + k] : ang[(r - 3) * n + k]; };
            auto qf = [&](int k) -> float & { return qr[k]; };
            for (int i = 0;; ++i) {
                float p[3], c[4], pos_err, rot_err;
                jac_loop(w, qr, 1, p, c, lin.data(), ang.data());
                // as the device kernels: a row whose q is not finite in ANY DoF, one off the link's chain included, gets a NaN error
                bool ok = true;
                for (int k = 0; k < n; ++k) ok = ok && std::isfinite(qr[k]);
                if (!ok) p[0] = NAN;
                if (drm::ik_iteration(J, n, p, c, target_pos + b * 3, tq, pos_only, o, i == max_iters, qf, lower, upper, pos_err, rot_err)) {
                    err[b * 2] = pos_err;
                    err[b * 2 + 1] = rot_err;
                    if (iters) iters[b] = i;
                    break;
                }
            }
        }
    });
    return DRM_OK;
}

// Operational-space dynamics of one link: every row runs jac_loop of the chain, crba_loop and rnea_loop (qdd = 0) of the tree, then
// drm_osc.hpp's arithmetic — the composed path of drm_osc.hip without its scratch
int64_t drm_operational_space_scratch_floats(const drm_walk *, const drm_walk *, int64_t) { return 0; }
int64_t drm_operational_space_scratch_floats_aligned(const drm_walk *, const drm_walk *, int64_t) { return 0; }

int drm_operational_space(const drm_walk *tree, const drm_walk *chain, const float *q, const float *qd, int64_t B, int32_t flags, float reg,
                          float *inertia, float *jbar, float *bias_acc, float *bias_force, float *, void *) {
    if (int rc = drm::args_operational_space(tree, chain, q, qd, B, reg, inertia, jbar, bias_acc, bias_force)) return rc;
    const bool pos_only = (flags & DRM_OSC_POSITION_ONLY) != 0;
    const float *qd_used = bias_acc || bias_force ? qd : nullptr;
    for_chunks(B, [&](int64_t, int64_t b0, int64_t rows) {
        if (pos_only) osc_host_rows<3>(tree, chain, q, qd_used, b0, rows, flags, reg * reg, inertia, jbar, bias_acc, bias_force);
        else osc_host_rows<6>(tree, chain, q, qd_used, b0, rows, flags, reg * reg, inertia, jbar, bias_acc, bias_force);
    });
    return DRM_OK;
}

// Forward-dynamics derivatives: every row runs fd_loop, crba_loop, n reverse sweeps of RNEA and drm_fdd.hpp's inverse and solves — the
// composed path of drm_fdd.hip without its scratch.  The walks drm_rnea_backward refuses are refused here, with its message.
int64_t drm_forward_dynamics_derivatives_scratch_floats(const drm_walk *, int64_t) { return 0; }
int64_t drm_forward_dynamics_derivatives_scratch_floats_aligned(const drm_walk *, int64_t) { return 0; }

int drm_forward_dynamics_derivatives(const drm_walk *w, const float *q, const float *qd, const float *f, int64_t B, int32_t flags,
                                     float *qdd, float *dq, float *dqd, float *minv, float *, void *) {
    if (int rc = drm::args_forward_dynamics_derivatives(w, q, qd, f, B, qdd, dq, dqd, minv)) return rc;
    const int fl = flags & (DRM_RNEA_GRAVITY | DRM_RNEA_DAMPING);
    for_chunks(B, [&](int64_t, int64_t b0, int64_t rows) { fdd_host_rows(w, q, qd, f, b0, rows, fl, qdd, dq, dqd, minv); });
    return DRM_OK;
}

// The inverse-dynamics regressor: every row runs drm_regressor.hpp's walk — the general kernel of drm_regressor.hip without its
// records in LDS / scratch.  The same walks are refused, with the same message.
int64_t drm_rnea_regressor_scratch_floats(const drm_walk *, int64_t) { return 0; }
int64_t drm_rnea_regressor_scratch_floats_aligned(const drm_walk *, int64_t) { return 0; }

int drm_rnea_regressor(const drm_walk *w, const float *q, const float *qd, const float *qdd, int64_t B, int32_t flags, float *Y, float *,
                       void *) {
    if (int rc = drm::args_rnea_regressor(w, q, qd, B, Y)) return rc;
    for_chunks(B, [&](int64_t, int64_t b0, int64_t rows) { regressor_host_rows(w, q, qd, qdd, b0, rows, flags, Y); });
    return DRM_OK;
}

// H, C and g of the equations of motion: every row runs drm_lagrangian.hpp's walk — the general kernel of drm_lagrangian.hip without its
// records in LDS / scratch.
int64_t drm_lagrangian_dynamics_scratch_floats(const drm_walk *, int64_t) { return 0; }
int64_t drm_lagrangian_dynamics_scratch_floats_aligned(const drm_walk *, int64_t) { return 0; }

int drm_lagrangian_dynamics(const drm_walk *w, const float *q, const float *qd, int64_t B, int32_t, float *H, float *C, float *g, float *,
                            void *) {
    if (int rc = drm::args_sweep_q_qd(w, q, qd, B, H || C || g)) return rc;
    for_chunks(B, [&](int64_t, int64_t b0, int64_t rows) { lagrangian_host_rows(w, q, qd, b0, rows, H, C, g); });
    return DRM_OK;
}

// Inverse dynamics and its first-order derivatives: every row runs drm_idd.hpp's walk — the general kernel of drm_idd.hip without its
// records in LDS / scratch.
int64_t drm_rnea_derivatives_scratch_floats(const drm_walk *, int64_t) { return 0; }
int64_t drm_rnea_derivatives_scratch_floats_aligned(const drm_walk *, int64_t) { return 0; }

int drm_rnea_derivatives(const drm_walk *w, const float *q, const float *qd, const float *qdd, int64_t B, int32_t flags, float *tau, float *dq,
                         float *dqd, float *H, float *, void *) {
    if (int rc = drm::args_rnea_derivatives(w, q, qd, qdd, B, tau, dq, dqd, H)) return rc;
    for_chunks(B, [&](int64_t, int64_t b0, int64_t rows) { idd_host_rows(w, q, qd, qdd, b0, rows, flags, tau, dq, dqd, H); });
    return DRM_OK;
}

// T, V, p, dT/dq and g: every row runs drm_energy.hpp's walk — the general kernel of drm_energy.hip without its records in LDS / scratch.
int64_t drm_energy_scratch_floats(const drm_walk *, int64_t) { return 0; }
int64_t drm_energy_scratch_floats_aligned(const drm_walk *, int64_t) { return 0; }

int drm_energy(const drm_walk *w, const float *q, const float *qd, int64_t B, int32_t, float *T, float *V, float *p, float *dT, float *g,
               float *, void *) {
    if (int rc = drm::args_sweep_q_qd(w, q, qd, B, T || V || p || dT || g)) return rc;
    for_chunks(B, [&](int64_t, int64_t b0, int64_t rows) { energy_host_rows(w, q, qd, b0, rows, T, V, p, dT, g); });
    return DRM_OK;
}

// Link motion and external-wrench torques: every row runs drm_links.hpp's arithmetic — the chain form where drm_links.hip would launch
// its fused kernels, the general walk elsewhere — without the state in LDS / scratch.
int64_t drm_link_motion_scratch_floats(const drm_walk *, int64_t) { return 0; }
int64_t drm_link_motion_scratch_floats_aligned(const drm_walk *, int64_t) { return 0; }
int64_t drm_external_torques_scratch_floats(const drm_walk *, int64_t) { return 0; }
int64_t drm_external_torques_scratch_floats_aligned(const drm_walk *, int64_t) { return 0; }

int drm_link_motion(const drm_walk *w, const float *q, const float *qd, const float *qdd, int64_t B, int32_t T, int32_t flags, float *pos,
                    float *lv, float *av, float *la, float *aa, float *, void *) {
    if (int rc = drm::args_link_motion(w, q, B, T, pos, lv, av, la, aa)) return rc;
    const int mode = (la || aa) ? 2 : (lv || av) ? 1 : 0;
    for_chunks(B, [&](int64_t, int64_t b0, int64_t rows) {
        if (mode == 2) link_motion_host_rows<2>(w, q, qd, qdd, b0, rows, T, flags, pos, lv, av, la, aa);
        else if (mode == 1) link_motion_host_rows<1>(w, q, qd, qdd, b0, rows, T, flags, pos, lv, av, la, aa);
        else link_motion_host_rows<0>(w, q, qd, qdd, b0, rows, T, flags, pos, lv, av, la, aa);
    });
    return DRM_OK;
}

int drm_external_torques(const drm_walk *w, const float *q, const float *force, const float *torque, int64_t B, int32_t T, int32_t flags,
                         float *tau, float *, void *) {
    if (int rc = drm::args_external_torques(w, q, force, torque, B, T, tau)) return rc;
    for_chunks(B, [&](int64_t, int64_t b0, int64_t rows) { link_torques_host_rows(w, q, force, torque, b0, rows, T, flags, tau); });
    return DRM_OK;
}

int64_t drm_link_power_dq_scratch_floats(const drm_walk *, int64_t) { return 0; }
int64_t drm_link_power_dq_scratch_floats_aligned(const drm_walk *, int64_t) { return 0; }
int drm_link_power_dq(const drm_walk *w, const float *q, const float *qd, const float *force, const float *torque, int64_t B, int32_t T,
                      int32_t flags, float *dq, float *tau, float *, void *) {
    if (int rc = drm::args_link_power_dq(w, q, qd, force, torque, B, T, dq)) return rc;
    for_chunks(B, [&](int64_t, int64_t b0, int64_t rows) { link_power_dq_host_rows(w, q, qd, force, torque, b0, rows, T, flags, dq, tau); });
    return DRM_OK;
}

// Contact torques and contact rollouts (drm_contact.hpp): every chunk of rows runs contact_host_rows, a rollout then fd_loop and the
// integrator of drm_rollout.hpp per step, the state of step t read back from the slab step t - 1 wrote.
int64_t drm_contact_torques_scratch_floats(const drm_walk *, int64_t) { return 0; }
int64_t drm_contact_torques_scratch_floats_aligned(const drm_walk *, int64_t) { return 0; }
int64_t drm_contact_rollout_scratch_floats(const drm_walk *, const drm_walk *, int64_t) { return 0; }
int64_t drm_contact_rollout_scratch_floats_aligned(const drm_walk *, const drm_walk *, int64_t) { return 0; }

int drm_contact_torques(const drm_walk *lw, const float *q, const float *qd, int64_t B, int32_t T, const drm_contact_plane *plane,
                        const float *radius, const drm_joint_springs *springs, const float *lower, const float *upper, int32_t flags,
                        float *tau, float *force, float *moment, float *, void *) {
    ContactPlan a;
    if (int rc = drm::args_contact_torques(lw, q, qd, B, T, plane, radius, springs, lower, upper, tau, a)) return rc;
    const int n = lw->n_dofs;
    for_chunks(B, [&](int64_t, int64_t b0, int64_t rows) {
        contact_host_rows(lw, a, q + b0 * n, qd + b0 * n, nullptr, rows, T, n, flags, true, tau + b0 * n,
                          force ? force + b0 * T * 3 : nullptr, moment ? moment + b0 * T * 3 : nullptr);
    });
    return DRM_OK;
}

int64_t drm_contact_torques_vjp_scratch_floats(const drm_walk *, int64_t) { return 0; }
int64_t drm_contact_torques_vjp_scratch_floats_aligned(const drm_walk *, int64_t) { return 0; }
int drm_contact_torques_vjp(const drm_walk *lw, const float *q, const float *qd, const float *grad_tau, int64_t B, int32_t T,
                            const drm_contact_plane *plane, const float *radius, const drm_joint_springs *springs, const float *lower,
                            const float *upper, int32_t flags, float *grad_q, float *grad_qd, float *, void *) {
    ContactPlan a;
    if (int rc = drm::args_contact_torques_vjp(lw, q, qd, grad_tau, B, T, plane, radius, springs, lower, upper, grad_q, grad_qd, a)) return rc;
    const int n = lw->n_dofs;
    for_chunks(B, [&](int64_t, int64_t b0, int64_t rows) {
        contact_vjp_host_rows(lw, a, q + b0 * n, qd + b0 * n, grad_tau + b0 * n, rows, T, n, flags, grad_q ? grad_q + b0 * n : nullptr,
                              grad_qd ? grad_qd + b0 * n : nullptr);
    });
    return DRM_OK;
}

// Collision cost and sphere distances (drm_collision.hpp): every chunk of rows runs collision_host_rows.
int64_t drm_collision_cost_scratch_floats(const drm_walk *, int64_t, int32_t) { return 0; }
int64_t drm_collision_cost_scratch_floats_aligned(const drm_walk *, int64_t, int32_t, int32_t, int32_t, int32_t) { return 0; }
int64_t drm_sphere_distances_scratch_floats(const drm_walk *, int64_t, int32_t) { return 0; }
int64_t drm_sphere_distances_scratch_floats_aligned(const drm_walk *, int64_t, int32_t, int32_t, int32_t, int32_t) { return 0; }

int drm_collision_cost(const drm_walk *w, const float *q, int64_t B, int32_t T, const drm_collision_spheres *spheres,
                       const drm_collision_world *world, const drm_collision_pairs *pairs, const drm_collision_params *params, int32_t flags,
                       float *cost, float *dq, float *, void *) {
    drm::CollTables t;
    if (int rc = drm::args_collision_cost(w, q, B, T, spheres, world, pairs, params, cost, dq, t)) return rc;
    const int n = w->n_dofs;
    for_chunks(B, [&](int64_t, int64_t b0, int64_t rows) {
        collision_host_rows(w, t, q + b0 * n, rows, flags, cost ? cost + b0 : nullptr, dq ? dq + b0 * n : nullptr, nullptr, nullptr, nullptr);
    });
    return DRM_OK;
}

int drm_sphere_distances(const drm_walk *w, const float *q, int64_t B, int32_t T, const drm_collision_spheres *spheres,
                         const drm_collision_world *world, const drm_collision_pairs *pairs, int32_t flags, float *center, float *wd,
                         float *sd, float *, void *) {
    drm::CollTables t;
    if (int rc = drm::args_sphere_distances(w, q, B, T, spheres, world, pairs, center, wd, sd, t)) return rc;
    const int n = w->n_dofs, S = t.S;
    for_chunks(B, [&](int64_t, int64_t b0, int64_t rows) {
        collision_host_rows(w, t, q + b0 * n, rows, flags, nullptr, nullptr, center ? center + b0 * S * 3 : nullptr, wd ? wd + b0 * S : nullptr,
                            sd ? sd + b0 * S : nullptr);
    });
    return DRM_OK;
}

int drm_contact_rollout(const drm_walk *dw, const drm_walk *lw, const float *q0, const float *qd0, const float *tau, int64_t B, int32_t T,
                        float dt, int32_t flags, int32_t TL, const drm_contact_plane *plane, const float *radius,
                        const drm_joint_springs *springs, const float *lower, const float *upper, float *q_traj, float *qd_traj,
                        float *qdd_traj, float *, void *) {
    ContactPlan a;
    if (int rc = drm::args_contact_rollout(dw, lw, q0, qd0, tau, B, T, dt, TL, plane, radius, springs, lower, upper, q_traj, qd_traj, a)) return rc;
    const int n = dw->n_dofs, fd_flags = flags & (DRM_RNEA_GRAVITY | DRM_RNEA_DAMPING);
    const bool expl = (flags & DRM_ROLLOUT_EXPLICIT_EULER) != 0;
    const int64_t slab = B * n;
    for_chunks(B, [&](int64_t, int64_t b0, int64_t rows) {
        std::vector<float> acc(qdd_traj ? 0 : (size_t)rows * n), total((size_t)rows * n);
        for (int t = 0; t < T; ++t) {
            const int64_t off = (int64_t)t * slab + b0 * n;
            const float *qi = t ? q_traj + off - slab : q0 + b0 * n, *qdi = t ? qd_traj + off - slab : qd0 + b0 * n;
            float *ac = qdd_traj ? qdd_traj + off : acc.data();
            contact_host_rows(lw, a, qi, qdi, tau + off, rows, TL, n, flags, false, total.data(), nullptr, nullptr);
            fd_loop(dw, qi, qdi, total.data(), rows, fd_flags, ac);
            for (int64_t i = 0; i < rows * n; ++i) {
                float x = qi[i], v = qdi[i];
                drm::rollout_step(x, v, ac[i], dt, expl);
                q_traj[off + i] = x;
                qd_traj[off + i] = v;
            }
        }
    });
    return DRM_OK;
}

// backward scratch: one [capacity, DRM_OPF_STRIDE] partial of the constant gradients per chunk of rows
int64_t drm_fk_backward_scratch_floats(int64_t B, int32_t capacity) {
    if (B < 0 || capacity < 1 || capacity > DRM_MAX_OPS) return 0;
    return n_chunks(B) * capacity * DRM_OPF_STRIDE;
}
int64_t drm_fk_mse_scratch_floats(int64_t B, int32_t capacity) {
    if (B < 0 || capacity < 1 || capacity > DRM_MAX_OPS) return 0;
    return n_chunks(B) * ((int64_t)capacity * DRM_OPF_STRIDE + 2); // + the chunk's part of the loss (a double)
}
int64_t drm_rnea_backward_scratch_floats(int64_t B, int32_t capacity, int32_t, int32_t) {
    return drm_fk_backward_scratch_floats(B, capacity);
}

int drm_fk_backward(const drm_walk *w, const float *q, int64_t B, int32_t T, const float *gpos, const float *grot, uint64_t mask,
                    float *gq, float *gops, float *scratch, void *) {
    if (int rc = drm::args_fk_backward(w, q, B, T, gpos, mask, gq, gops)) return rc;
    if (mask && !scratch) return fail(DRM_ERR_INVALID, "scratch must not be NULL (drm_fk_backward_scratch_floats)");
    const int n = w->n_dofs, entries = w->capacity * DRM_OPF_STRIDE;
    for_chunks(B, [&](int64_t c, int64_t b0, int64_t rows) {
        fkb_t(w, q + b0 * n, rows, T, gpos + b0 * T * 3, nullptr, nullptr, mask, gq ? gq + b0 * n : nullptr,
              mask ? scratch + c * entries : nullptr, grot ? grot + b0 * T * 9 : nullptr);
    });
    if (mask) reduce_partials(scratch, n_chunks(B), entries, gops);
    return DRM_OK;
}

int drm_fk_jacobian_backward(const drm_walk *w, const float *q, int64_t B, const float *gpos, const float *grot, const float *glin,
                             const float *gang, uint64_t mask, float *gq, float *gops, float *scratch, void *) {
    if (int rc = drm::args_fk_jacobian_backward(w, q, B, glin, gang, mask, gq, gops)) return rc;
    if (mask && !scratch) return fail(DRM_ERR_INVALID, "scratch must not be NULL (drm_fk_backward_scratch_floats)");
    const int n = w->n_dofs, entries = w->capacity * DRM_OPF_STRIDE;
    for_chunks(B, [&](int64_t c, int64_t b0, int64_t rows) {
        fkb_t(w, q + b0 * n, rows, 1, gpos ? gpos + b0 * 3 : nullptr, glin + b0 * 3 * n, gang + b0 * 3 * n, mask,
              gq ? gq + b0 * n : nullptr, mask ? scratch + c * entries : nullptr, grot ? grot + b0 * 9 : nullptr);
    });
    if (mask) reduce_partials(scratch, n_chunks(B), entries, gops);
    return DRM_OK;
}

// forward pose, loss and adjoints chunk by chunk (any single-target walk, any B: the host build has no tile shape to respect)
int drm_fk_mse(const drm_walk *w, const float *q, const float *target, int64_t B, uint64_t mask, float *loss, float *gq, float *gops,
               float *scratch, void *) {
    if (int rc = drm::args_fk_mse(w, q, target, mask, loss, gops, scratch)) return rc;
    if (B < 1) return fail(DRM_ERR_INVALID, "drm_fk_mse: the loss is a mean over at least one row");
    const int n = w->n_dofs, entries = w->capacity * DRM_OPF_STRIDE;
    const int64_t chunks = n_chunks(B), stride = entries + 2;
    const float g_scale = 2.0f / (3.0f * (float)B);
    for_chunks(B, [&](int64_t c, int64_t b0, int64_t rows) {
        float pos[CHUNK * 3], quat[CHUNK * 4], g[CHUNK * 3];
        fk_loop(w, q + b0 * n, rows, 1, pos, quat);
        double part = 0.0;
        for (int64_t i = 0; i < rows * 3; ++i) {
            const float d = pos[i] - target[b0 * 3 + i];
            part += (double)d * d;
            g[i] = d * g_scale;
        }
        memcpy(scratch + c * stride + entries, &part, sizeof(double));
        fkb_t(w, q + b0 * n, rows, 1, g, nullptr, nullptr, mask, gq ? gq + b0 * n : nullptr, mask ? scratch + c * stride : nullptr);
    });
    double total = 0.0;
    for (int64_t c = 0; c < chunks; ++c) {
        double part;
        memcpy(&part, scratch + c * stride + entries, sizeof(double));
        total += part;
    }
    loss[0] = (float)(total / (3.0 * (double)B));
    if (mask)
        for (int e = 0; e < entries; ++e) {
            double s = 0.0;
            for (int64_t c = 0; c < chunks; ++c) s += scratch[c * stride + e];
            gops[e] = (float)s;
        }
    return DRM_OK;
}

int drm_rnea_backward(const drm_walk *w, const float *q, const float *qd, const float *qdd, int64_t B, int32_t flags, const float *gtau,
                      uint64_t mask, float *gq, float *gqd, float *gqdd, float *gops, float *scratch, void *) {
    if (int rc = drm::args_rnea_backward(w, q, qd, B, gtau, mask, gq, gqd, gqdd, gops)) return rc;
    if (mask && !scratch) return fail(DRM_ERR_INVALID, "scratch must not be NULL (drm_rnea_backward_scratch_floats)");
    const int n = w->n_dofs, entries = w->capacity * DRM_OPF_STRIDE;
    for_chunks(B, [&](int64_t c, int64_t b0, int64_t rows) {
        rneab_t(w, q + b0 * n, qd + b0 * n, qdd ? qdd + b0 * n : nullptr, rows, flags, gtau + b0 * n, mask, gq ? gq + b0 * n : nullptr,
                gq ? gqd + b0 * n : nullptr, gq ? gqdd + b0 * n : nullptr, mask ? scratch + c * entries : nullptr);
    });
    if (mask) reduce_partials(scratch, n_chunks(B), entries, gops);
    return DRM_OK;
}

int drm_link_rows(const float *params, int32_t n_links, float *rows, void *) {
    if (int rc = drm::args_link_rows(params, n_links, rows)) return rc;
    for (int i = 0; i < n_links; ++i) link_row(params + i * LINK_PARAM_FLOATS, rows + i * DRM_OPF_STRIDE);
    return DRM_OK;
}
int drm_link_rows_backward(const float *params, const float *grad_rows, int32_t n_links, float *grad_params, void *) {
    if (int rc = drm::args_link_rows_backward(params, grad_rows, n_links, grad_params)) return rc;
    for (int i = 0; i < n_links; ++i)
        link_row_backward(params + i * LINK_PARAM_FLOATS, grad_rows + i * DRM_OPF_STRIDE, grad_params + i * LINK_PARAM_FLOATS);
    return DRM_OK;
}

int drm_walk_table(const float *params, int32_t n_links, const float *base, const int32_t *sel, const float *gsign, int32_t n_entries,
                   float *ops_f, void *) {
    if (int rc = drm::args_walk_table("drm_walk_table", params, n_links, base, sel, gsign, n_entries, ops_f)) return rc;
    float rows[32 * DRM_OPF_STRIDE];
    for (int i = 0; i < n_links; ++i) link_row(params + i * LINK_PARAM_FLOATS, rows + i * DRM_OPF_STRIDE);
    for (int e = 0; e < n_entries; ++e) {
        const int r = sel[e];
        if (r >= n_links * DRM_OPF_STRIDE) return fail(DRM_ERR_INVALID, "sel[%s%ld] = %ld is beyond the learnable rows", "", e, r);
        ops_f[e] = r >= 0 ? rows[r] * gsign[e] : base[e];
    }
    return DRM_OK;
}
int drm_walk_table_backward(const float *params, int32_t n_links, const float *grad_ops_f, const int32_t *sel, const float *gsign,
                            int32_t n_entries, float *grad_params, void *) {
    if (int rc = drm::args_walk_table("drm_walk_table_backward", params, n_links, grad_ops_f, sel, gsign, n_entries, grad_params)) return rc;
    float grows[32 * DRM_OPF_STRIDE];
    for (int r = 0; r < n_links * DRM_OPF_STRIDE; ++r) grows[r] = 0.0f;
    for (int e = 0; e < n_entries; ++e) { // entry order, as the kernel adds them
        const int r = sel[e];
        if (r >= 0 && r < n_links * DRM_OPF_STRIDE) grows[r] += grad_ops_f[e] * gsign[e];
    }
    for (int i = 0; i < n_links; ++i)
        link_row_backward(params + i * LINK_PARAM_FLOATS, grows + i * DRM_OPF_STRIDE, grad_params + i * LINK_PARAM_FLOATS);
    return DRM_OK;
}

// ABI 13: the table from the links' parameter tensors where they lie, in the forms their modules store them, and the gradient back
// to those tensors (include/drm_hip.h)
// the pieces and forms of CHECKED links (drm_args.hpp args_walk_table_links) read into drm_link_rows' layout
static void links_raw(const drm_link_pieces *links, const drm_link_forms *forms, int32_t n_links, float *raw, int32_t (*form)[3], float (*c)[3]) {
    for (int l = 0; l < n_links; ++l) {
        const float *at[6] = {links[l].rot_angles, links[l].trans, links[l].mass, links[l].com, links[l].inertia_mat, links[l].damping};
        const drm_link_forms f = forms ? forms[l] : drm_link_forms{};
        form[l][0] = f.mass; form[l][1] = f.inertia_mat; form[l][2] = f.damping;
        c[l][0] = f.mass_c; c[l][1] = f.inertia_mat_c; c[l][2] = f.damping_c;
        for (int k = 0; k < LINK_PARAM_FLOATS; ++k) {
            const int piece = link_piece_of(k), off = link_piece_offset(k);
            const bool there = piece != 4 || f.inertia_mat == DRM_FORM_PLAIN || off < 6;
            raw[l * LINK_PARAM_FLOATS + k] = there ? at[piece][off] : 0.0f;
        }
    }
}
int drm_walk_table_links(const drm_link_pieces *links, const drm_link_forms *forms, int32_t n_links, const float *base, const int32_t *sel,
                         const float *gsign, int32_t n_entries, float *ops_f, void *) {
    float raw[32 * LINK_PARAM_FLOATS], params[32 * LINK_PARAM_FLOATS], c[32][3];
    int32_t form[32][3];
    if (int rc = drm::args_walk_table_links("drm_walk_table_links", links, forms, n_links, base, sel, gsign, n_entries, ops_f)) return rc;
    links_raw(links, forms, n_links, raw, form, c);
    for (int l = 0; l < n_links; ++l) link_forms_apply(form[l], c[l], raw + l * LINK_PARAM_FLOATS, params + l * LINK_PARAM_FLOATS);
    return drm_walk_table(params, n_links, base, sel, gsign, n_entries, ops_f, nullptr);
}
int drm_walk_table_links_backward(const drm_link_pieces *links, const drm_link_forms *forms, int32_t n_links, const float *grad_ops_f,
                                  const int32_t *sel, const float *gsign, int32_t n_entries, float *grad_params, void *) {
    float raw[32 * LINK_PARAM_FLOATS], params[32 * LINK_PARAM_FLOATS], c[32][3];
    int32_t form[32][3];
    if (int rc = drm::args_walk_table_links("drm_walk_table_links_backward", links, forms, n_links, grad_ops_f, sel, gsign, n_entries, grad_params))
        return rc;
    links_raw(links, forms, n_links, raw, form, c);
    for (int l = 0; l < n_links; ++l) link_forms_apply(form[l], c[l], raw + l * LINK_PARAM_FLOATS, params + l * LINK_PARAM_FLOATS);
    if (int rc = drm_walk_table_backward(params, n_links, grad_ops_f, sel, gsign, n_entries, grad_params, nullptr)) return rc;
    for (int l = 0; l < n_links; ++l) link_forms_grad(form[l], raw + l * LINK_PARAM_FLOATS, grad_params + l * LINK_PARAM_FLOATS);
    return DRM_OK;
}

// ABI 12: the composition itself (the host build has no launches to save): table from the links' parameters, drm_fk_mse, and the
// gradient back through the table's map
int drm_fk_mse_links(const drm_walk *w, const int32_t *sel, const float *gsign, const drm_link_pieces *links, int32_t n_links, const float *q,
                     const float *target, int64_t B, uint64_t mask, float *loss, float *gq, float *grad_params, float *scratch, void *) {
    if (int rc = drm::args_fk_mse_links(w, sel, gsign, links, n_links, q, target, mask, loss, grad_params, scratch)) return rc;
    const int entries = w->capacity * DRM_OPF_STRIDE;
    float params[DRM_FK_MSE_MAX_LINKS * LINK_PARAM_FLOATS] = {0.0f};
    for (int l = 0; l < n_links; ++l) {
        for (int i = 0; i < 3; ++i) {
            params[l * LINK_PARAM_FLOATS + i] = links[l].rot_angles[i];
            params[l * LINK_PARAM_FLOATS + 3 + i] = links[l].trans[i];
        }
    }
    std::vector<float> table(entries), gops(entries);
    if (int rc = drm_walk_table(params, n_links, w->ops_f, sel, gsign, entries, table.data(), nullptr)) return rc;
    drm_walk live = *w;
    live.ops_f = table.data();
    if (int rc = drm_fk_mse(&live, q, target, B, mask, loss, gq, gops.data(), scratch, nullptr)) return rc;
    for (int e = 0; e < entries; ++e)       // forward kinematics reads the FT block of a row only
        if ((e % DRM_OPF_STRIDE) >= DRM_OPF_FT_FLOATS) gops[e] = 0.0f;
    if (int rc = drm_walk_table_backward(params, n_links, gops.data(), sel, gsign, entries, grad_params, nullptr)) return rc;
    for (int l = 0; l < n_links; ++l)
        for (int i = 6; i < LINK_PARAM_FLOATS; ++i) grad_params[l * LINK_PARAM_FLOATS + i] = 0.0f;
    return DRM_OK;
}
} // extern "C"

// ---- include/drm_hip_whole_body.h ---------------------------------------------------------------------------------------------------
namespace {
// the walks drm_whole_body.hip's fused kernel takes.  The host build runs its straight-line arithmetic (drm_whole_body.hpp
// whole_body_chain_trig) on every row of such a call, the general walk with DRM_WHOLE_BODY_COMPOSED.
bool whole_body_chain_walk(const drm_walk *w, int flags) {
    return !(flags & DRM_WHOLE_BODY_COMPOSED) && (w->shape & DRM_WALK_ARM_CHAIN) && w->capacity == 8 && w->n_dofs == 7;
}
// drm_whole_body, rows [b0, b0 + rows): drm_whole_body.hpp's walk of the row, its records on this thread's heap
template <int LEVEL>
void whole_body_host_rows(const drm_walk *w, const float *q, const float *qd, const float *qdd, int64_t b0, int64_t rows, int flags,
                          const float *base, float *com, float *com_vel, float *com_acc, float *com_jac, float *ang_mom, float *force,
                          float *moment) {
    const int n = w->n_dofs, n_ops = w->n_ops, n_slots = w->n_slots;
    const Ctl ctl(w);
    HostRecords<drm::wb_rec_floats(LEVEL)> rec(n_ops); HostRecords<drm::wb_slot_floats(LEVEL)> slots(n_slots);
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const bool chain = whole_body_chain_walk(w, flags), gravity = (flags & DRM_RNEA_GRAVITY) != 0;
    const int links = w->n_ops == w->n_dofs ? 7 : 8;
    auto row = [&](int k) { return w->ops_f + k * DRM_OPF_STRIDE; };
    for (int64_t b = b0; b < b0 + rows; ++b) {
        const float *qr = q + b * n, *qdr = (LEVEL >= 1 && qd) ? qd + b * n : nullptr, *qddr = (LEVEL >= 2 && qdd) ? qdd + b * n : nullptr;
        float *jr = com_jac ? com_jac + b * 3 * n : nullptr;
        bool bad = false;
        for (int d = 0; d < n; ++d) bad = bad || drm::wb_bad_input(qr[d], qdr ? qdr[d] : 0.0f, qddr ? qddr[d] : 0.0f);
        drm::WbRoot root;
        if (chain) {
            float qv[7], qdv[7], qddv[7], cs[7], sn[7], jac[21];
            for (int d = 0; d < 7; ++d) {
                qv[d] = bad ? 0.0f : qr[d];
                qdv[d] = (bad || !qdr) ? 0.0f : qdr[d];
                qddv[d] = (bad || !qddr) ? 0.0f : qddr[d];
            }
            drm::chain_trig<7>(qv, cs, sn);
            if (jr && links == 7) drm::whole_body_chain_trig<7, 7, LEVEL, true>(row, cs, sn, qdv, qddv, jac, base[0], root);
            else if (jr) drm::whole_body_chain_trig<8, 7, LEVEL, true>(row, cs, sn, qdv, qddv, jac, base[0], root);
            else if (links == 7) drm::whole_body_chain_trig<7, 7, LEVEL, false>(row, cs, sn, qdv, qddv, jac, base[0], root);
            else drm::whole_body_chain_trig<8, 7, LEVEL, false>(row, cs, sn, qdv, qddv, jac, base[0], root);
            if (jr)
                for (int i = 0; i < 21; ++i) jr[i] = bad ? nan : jac[i];
        } else {
            drm::whole_body_tree_walk<LEVEL>(
                n_ops, w->n_segments > 1 ? w->prefix_end : 0, n_slots, ctl, row,
                [&](int d, float &a, float &v, float &acc) {
                    a = bad ? 0.0f : qr[d];
                    v = (bad || !qdr) ? 0.0f : qdr[d];
                    acc = (bad || !qddr) ? 0.0f : qddr[d];
                },
                [&](int k, const float *x) { rec.put(k, x); }, [&](int k, float *x) { rec.get(k, x); },
                [&](int s, const float *x) { slots.put(s, x); }, [&](int s, float *x) { slots.get(s, x); },
                [&](int j, const float *col) {
                    if (j >= n || !jr) return;
                    for (int i = 0; i < 3; ++i) jr[i * n + j] = bad ? nan : col[i];
                },
                base[0], root);
        }
        drm::WbOut o;
        drm::wb_finish<LEVEL>(root, base, gravity, o);
        for (int i = 0; i < 3; ++i) {
            if (com) com[b * 3 + i] = bad ? nan : o.com[i];
            if (LEVEL >= 1 && com_vel) com_vel[b * 3 + i] = bad ? nan : o.com_vel[i];
            if (LEVEL >= 2 && com_acc) com_acc[b * 3 + i] = bad ? nan : o.com_acc[i];
            if (LEVEL >= 1 && ang_mom) ang_mom[b * 3 + i] = bad ? nan : o.ang_mom[i];
            if (force) force[b * 3 + i] = bad ? nan : o.force[i];
            if (moment) moment[b * 3 + i] = bad ? nan : o.moment[i];
        }
    }
}
} // namespace

extern "C" {
// The centre of mass, its Jacobian, momentum and the base wrench: every row runs drm_whole_body.hpp's arithmetic — the chain form where
// drm_whole_body.hip would launch its fused kernel, the general walk elsewhere — without the records in LDS / scratch.
int64_t drm_whole_body_scratch_floats(const drm_walk *, int64_t) { return 0; }
int64_t drm_whole_body_scratch_floats_aligned(const drm_walk *, int64_t) { return 0; }

int drm_whole_body(const drm_walk *w, const float *q, const float *qd, const float *qdd, int64_t B, int32_t flags, const drm_base_share *base,
                   float *com, float *com_vel, float *com_acc, float *com_jac, float *ang_mom, float *force, float *moment, float *, void *) {
    drm::WholeBodyBase hb;
    if (int rc = drm::args_whole_body(w, q, qd, B, base, com, com_vel, com_acc, com_jac, ang_mom, force, moment, hb)) return rc;
    const int level = drm::whole_body_level(qd, qdd, com_vel, com_acc, ang_mom, force, moment);
    for_chunks(B, [&](int64_t, int64_t b0, int64_t rows) {
        if (level == 2) whole_body_host_rows<2>(w, q, qd, qdd, b0, rows, flags, hb.v, com, com_vel, com_acc, com_jac, ang_mom, force, moment);
        else if (level == 1) whole_body_host_rows<1>(w, q, qd, qdd, b0, rows, flags, hb.v, com, com_vel, com_acc, com_jac, ang_mom, force, moment);
        else whole_body_host_rows<0>(w, q, qd, qdd, b0, rows, flags, hb.v, com, com_vel, com_acc, com_jac, ang_mom, force, moment);
    });
    return DRM_OK;
}
} // extern "C"
