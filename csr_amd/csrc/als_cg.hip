// The ALS half-step by conjugate gradient for libcsrk on gfx950: per row of a CSR matrix, a fixed number of CG steps on the
// row's normal equations without ever forming the k x k block (include/csrk.h, rule C).
//     csrk_als_rows_cg    per row i: M_i = base + sum_e w_e v_e v_e^T + (lam + lam_n n_i) I is applied, never built:
//                         M y = base y + rho y + sum_e v_e (w_e (v_e . y)), one pass over the row's V rows per product
// Where csrk_als_rows pays n k^2 / 2 fused multiply-adds to build the block and k^3 / 6 to factorise it, a step here is a
// dot and an axpy per entry (4 k flops) plus, with a base, one k x k matrix-vector product.
//
// Work split.  ONE 16-LANE TEAM (one DPP row) PER ROW OF THE MATRIX, at every k: four rows per wavefront, sixteen per
// workgroup.  Lane l owns the columns of csrk_sddmm's partial l (in each 64-column chunk: float64 2 l, 2 l + 1, 32 + 2 l,
// 33 + 2 l; float32 4 l .. 4 l + 3: panel_off and panel_load4 in device_loads.h, the code SDDMM runs), so a V row
// arrives in 16-B pieces, each load instruction of a team one contiguous
// 256-B span, and x, r, p, q and b live in registers: 4 doubles each per chunk and lane, 8 at k = 128.  A DOT is the
// lane's fma chain over its columns and four DPP adds; the adds form a butterfly (lane ^ 1, ^ 2, then the half-row and
// row mirrors), so EVERY lane ends with the sum in rule C2's tree shape -- floating-point addition commutes, so the lanes
// agree bit for bit (NaN payloads apart) -- and no broadcast follows.  CG_E entries' V rows are loaded, and their dots
// taken, before the first is used; only the one-fma-per-entry chain into q_t is serial.  No LDS in the entry loop.
//
// base (k x k, read as stored: element (t, u) is base[u k + t]) is streamed per team, row u in the same 16-B pieces (the
// sixteen teams of a workgroup walk it in near step: the CU's vector cache serves most of it), and y_u is read from k
// doubles of LDS per team that the team published just before: teams are parts of one wavefront, so the publication needs
// no workgroup barrier.  That is the only LDS: 16 KB per workgroup at k = 128.
//
// Long rows.  A team walks its row CG_E entries per round trip, steps + 1 times (steps + 2 with an x0): a 250 000-entry
// row took 330-550 ms that way, most of the launch on a power-law matrix.  So a row of at least L entries
// (csrk_als_cg_set_long; rule C11) is not a team's: als_cg_long_kernel below gives it a whole workgroup, launched first
// on the same stream, and the team kernel returns from such a row before touching anything.  The same routines run in
// both, each chain is serial in both, so no bit depends on L; the 250 000-entry row alone takes 53-57 ms at k = 64
// (DESIGN.md section 7d has the table).  csrk_als_rows has a tail of its own (45-87 ms) and no such class.
//
// Divergence.  The teams of a wavefront have rows of different lengths and stop after different numbers of steps: every
// loop is team-uniform, and nothing crosses a team (the DPP controls stay inside a row of 16 lanes).
#include "common.h"
#include "device_loads.h"
#include "panel.h"
#include "team_dot.h"
#include "wave.h"
#include <atomic>
#include <cstdlib>

namespace csrk {

constexpr int CG_G = 16;                 // lanes per team (one DPP row)
static_assert(CG_G == PANEL_G, "a team is the lanes that share a panel row (device_loads.h)");
constexpr int CG_THREADS = 256;
constexpr int CG_TEAMS = CG_THREADS / CG_G;
constexpr int CG_E = 4;                  // entries in flight per team and step of the entry loop
constexpr int CG_K_MAX = 128;            // two chunks of 64 columns (csrk_als_limits' value)

// (rule C2's DOT, cg_dot, and its tree, cg_team_sum: team_dot.h)

// rule C3's first two parts: q = base y (u ascending), then q_t = fma(rho, y_t, q_t).  ys: the team's k doubles of LDS.
template <class OFFT, int NCH, bool BW>
__device__ __forceinline__ void cg_base_part(const double *__restrict__ base, int k, int sub, const double (&y)[NCH][4],
                                             double (&q)[NCH][4], double *ys)
{
    team_sync<CG_G>();                                                      // (the last product's reads of ys are done)
#pragma unroll
    for (int c = 0; c < NCH; c++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int t = 64 * c + panel_off<OFFT>(sub, i);
            if (t < k) ys[t] = y[c][i];
        }
    team_sync<CG_G>();
#pragma unroll 2
    for (int u = 0; u < k; u++) {
        const double yu = ys[u];
        double bv[NCH][4];
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            if (sizeof(OFFT) == 8) {
                panel_load4<double, BW>(base + (int64_t)u * k + 64 * c, sub, k - 64 * c, bv[c]);
            } else {                                                        // float32 ownership: columns 4 l .. 4 l + 3, two pieces of doubles
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const int o = 4 * sub + 2 * h;
                    if (BW && o + 2 <= k - 64 * c) {
                        panel_piece(base + (int64_t)u * k + 64 * c + o, bv[c] + 2 * h);
                    } else {
#pragma unroll
                        for (int i = 0; i < 2; i++) bv[c][2 * h + i] = o + i < k - 64 * c ? base[(int64_t)u * k + 64 * c + o + i] : 0.0;
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < NCH; c++)
#pragma unroll
            for (int i = 0; i < 4; i++) q[c][i] = __builtin_fma(bv[c][i], yu, q[c][i]);
    }
}

// q = M y without the entries' part; the walk adds that (rule C3)
template <class OFFT, int NCH>
__device__ __forceinline__ void cg_head(const double *__restrict__ base, bool bwide, double rho, int k, int sub,
                                        const double (&y)[NCH][4], double (&q)[NCH][4], double *ys)
{
#pragma unroll
    for (int c = 0; c < NCH; c++)
#pragma unroll
        for (int i = 0; i < 4; i++) q[c][i] = 0.0;
    if (base) {
        if (bwide) cg_base_part<OFFT, NCH, true>(base, k, sub, y, q, ys);
        else cg_base_part<OFFT, NCH, false>(base, k, sub, y, q, ys);
    }
#pragma unroll
    for (int c = 0; c < NCH; c++)
#pragma unroll
        for (int i = 0; i < 4; i++) q[c][i] = __builtin_fma(rho, y[c][i], q[c][i]);
}

// One pass over the row's entries in storage order, CG_E at a time.  WANT_B: b_t = fma(c_e, v_e[t], b_t) (rule C4).
// WANT_Q: d_e = DOT(v_e, y), g_e = round(w_e d_e) or d_e, q_t = fma(g_e, v_e[t], q_t) (rule C3's last part).
template <class T, bool WIDE, int NCH, bool WANT_B, bool WANT_Q>
__device__ __forceinline__ void cg_walk(int64_t e0, int64_t e1, const int32_t *__restrict__ ci, const void *__restrict__ vals, int vt,
                                        bool scaled, int rhs_mode, const T *__restrict__ V, int64_t ldv, int k, int sub,
                                        const double (&y)[NCH][4], double (&q)[NCH][4], double (&b)[NCH][4])
{
    if (e0 >= e1) return;
    const int64_t last = e1 - 1;
    int32_t coln[CG_E];                                                     // the next step's column indices
#pragma unroll
    for (int x = 0; x < CG_E; x++) coln[x] = ci[e0 + x < last ? e0 + x : last];
    for (int64_t es = e0; es < e1; es += CG_E) {
        T v[CG_E][NCH][4];
        double wv[CG_E], d[CG_E];
#pragma unroll
        for (int x = 0; x < CG_E; x++)                                      // (past the row: its last entry again, unused)
#pragma unroll
            for (int c = 0; c < NCH; c++) panel_load4<T, WIDE>(V + (int64_t)coln[x] * ldv + 64 * c, sub, k - 64 * c, v[x][c]);
#pragma unroll
        for (int x = 0; x < CG_E; x++) {
            const int64_t e = es + x < last ? es + x : last;
            wv[x] = vals ? csr_stored_val(vals, vt, e) : 1.0;
            const int64_t en = es + CG_E + x < last ? es + CG_E + x : last;
            coln[x] = ci[en];
        }
        if (WANT_Q) {
#pragma unroll
            for (int x = 0; x < CG_E; x++) d[x] = cg_dot<T, NCH>(v[x], y, sub, k);
        }
#pragma unroll
        for (int x = 0; x < CG_E; x++)
            if (es + x < e1) {
                if (WANT_Q) {
                    const double g = scaled ? __dmul_rn(wv[x], d[x]) : d[x];
#pragma unroll
                    for (int c = 0; c < NCH; c++)
#pragma unroll
                        for (int i = 0; i < 4; i++) q[c][i] = __builtin_fma(g, (double)v[x][c][i], q[c][i]);
                }
                if (WANT_B) {
                    const double cc = rhs_mode == CSRK_ALS_RHS_ONES ? 1.0 : (rhs_mode == CSRK_ALS_RHS_VALUES ? wv[x] : __dadd_rn(1.0, wv[x]));
#pragma unroll
                    for (int c = 0; c < NCH; c++)
#pragma unroll
                        for (int i = 0; i < 4; i++) b[c][i] = __builtin_fma(cc, (double)v[x][c][i], b[c][i]);
                }
            }
    }
}

// NCH chunks of 64 columns: k <= 64 NCH.  vals: NULL when no value is wanted or none is stored (every one 1.0).
template <class T, bool WIDE, int NCH>
__global__ __launch_bounds__(CG_THREADS) void als_cg_kernel(const void *__restrict__ rp, int ptr64, const int32_t *__restrict__ ci,
                                                            const void *__restrict__ vals, int vt, int scaled, int32_t row_begin,
                                                            int32_t row_end, const T *__restrict__ V, int64_t ldv, int32_t k,
                                                            int rhs_mode, const double *__restrict__ base, int bwide, double lam,
                                                            double lam_n, int32_t steps, double tol2, const double *x0, int64_t ldx0,
                                                            double *out, int64_t ldo, double *__restrict__ resid,
                                                            int32_t *__restrict__ taken_out, int64_t long_from)
{
    __shared__ __attribute__((aligned(16))) double ysh[CG_TEAMS][NCH * 64];
    const int team = threadIdx.x / CG_G, sub = threadIdx.x % CG_G;
    const int64_t row = (int64_t)row_begin + (int64_t)blockIdx.x * CG_TEAMS + team;
    if (row >= row_end) return;                                             // (a whole team; teams never meet at a barrier)
    const int64_t e0 = load_ptr(rp, ptr64, row), e1 = load_ptr(rp, ptr64, row + 1);
    if (e1 - e0 >= long_from) return;                                       // a long row: als_cg_long_kernel's, out and all
    const double rho = __builtin_fma(lam_n, (double)(e1 - e0), lam);
    double *ys = ysh[team];

    double x[NCH][4], r[NCH][4], p[NCH][4], q[NCH][4];
#pragma unroll
    for (int c = 0; c < NCH; c++)
#pragma unroll
        for (int i = 0; i < 4; i++) x[c][i] = 0.0, r[c][i] = 0.0, q[c][i] = 0.0;

    // rules C4 and C5: b, and with an x0 the first product, in one walk; r holds b, then b - q
    if (x0) {
        const double *xr = x0 + (int64_t)(row - row_begin) * ldx0;
#pragma unroll
        for (int c = 0; c < NCH; c++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int t = 64 * c + panel_off<T>(sub, i);
                x[c][i] = t < k ? xr[t] : 0.0;
            }
        cg_head<T, NCH>(base, bwide != 0, rho, k, sub, x, q, ys);
        cg_walk<T, WIDE, NCH, true, true>(e0, e1, ci, vals, vt, scaled != 0, rhs_mode, V, ldv, k, sub, x, q, r);
#pragma unroll
        for (int c = 0; c < NCH; c++)
#pragma unroll
            for (int i = 0; i < 4; i++) r[c][i] = __dsub_rn(r[c][i], q[c][i]);
    } else {
        cg_walk<T, WIDE, NCH, true, false>(e0, e1, ci, vals, vt, scaled != 0, rhs_mode, V, ldv, k, sub, x, q, r);
    }
#pragma unroll
    for (int c = 0; c < NCH; c++)
#pragma unroll
        for (int i = 0; i < 4; i++) p[c][i] = r[c][i];
    double rs = cg_dot<T, NCH>(r, r, sub, k);
    int32_t taken = 0;

    // rule C6
    while (taken < steps && rs > tol2) {
        cg_head<T, NCH>(base, bwide != 0, rho, k, sub, p, q, ys);
        cg_walk<T, WIDE, NCH, false, true>(e0, e1, ci, vals, vt, scaled != 0, rhs_mode, V, ldv, k, sub, p, q, r);
        const double pq = cg_dot<T, NCH>(p, q, sub, k);
        const double alpha = __ddiv_rn(rs, pq);
#pragma unroll
        for (int c = 0; c < NCH; c++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                x[c][i] = __builtin_fma(alpha, p[c][i], x[c][i]);
                r[c][i] = __builtin_fma(-alpha, q[c][i], r[c][i]);
            }
        const double rn = cg_dot<T, NCH>(r, r, sub, k);
        const double beta = __ddiv_rn(rn, rs);
#pragma unroll
        for (int c = 0; c < NCH; c++)
#pragma unroll
            for (int i = 0; i < 4; i++) p[c][i] = __builtin_fma(beta, p[c][i], r[c][i]);
        rs = rn;
        taken++;
    }

    double *o = out + (int64_t)(row - row_begin) * ldo;
#pragma unroll
    for (int c = 0; c < NCH; c++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int t = 64 * c + panel_off<T>(sub, i);
            if (t < k) o[t] = x[c][i];
        }
    if (sub == 0) {
        if (resid) resid[row - row_begin] = rs;
        if (taken_out) taken_out[row - row_begin] = taken;
    }
}

// ---- the long-row class (rule C11): one workgroup per row of at least `long_from` entries ------------------------------
// Team 0 (the first 16 lanes of wavefront 0) holds x, r, p, q and b exactly as a team of als_cg_kernel does and runs the
// same cg_dot / cg_head and step-C6 code.  Per product it publishes y to LDS; the LR_FILL_TEAMS teams of wavefronts 1..3
// read y into registers in that layout and fill: a chunk is LR_FILL_TEAMS x E consecutive entries, a team's E of them
// loaded with panel_load4 before the first is used; d_e = cg_dot(v_e, y), g_e and c_e go to small LDS arrays and v_e to
// an LDS image in the panel's type, written in the 16-B pieces it arrived in (a team's store is 256 contiguous bytes).
// Wavefront 0 owns the chains, column 64 c + lane per lane: it reads one 8-B (4-B) word per lane of the image row --
// consecutive addresses, no bank conflict -- and g_e, c_e as broadcasts, one fma per entry and column in storage order.
// The image is double-buffered: chunk i is chained while chunk i + 1 is filled, one workgroup barrier per chunk.  The
// head of q (base y + rho y) crosses from team 0's layout to the chain's and the finished q and b cross back through 2 k
// doubles of LDS inside wavefront 0.  Every loop is workgroup-uniform: team 0 publishes the stop decision.
constexpr int LR_THREADS = 256;
constexpr int LR_S = 1024;               // rows of the requested range whose lengths one workgroup scans
constexpr int LR_BUFS = 2;
constexpr int LR_FILL_TEAMS = (LR_THREADS - 64) / CG_G;
constexpr int LR_TEAM_BYTES = 4096;      // of V rows a fill team has in flight at most: 12 teams, 48 KB per workgroup
constexpr int LR_E_MAX = 8;              // ... and entries (their dots and values are registers too)
constexpr int64_t LR_DEFAULT_LONG = 2048;
template <class T, int NCH> constexpr int lr_e()
{
    return LR_TEAM_BYTES / (NCH * 64 * (int)sizeof(T)) < LR_E_MAX ? LR_TEAM_BYTES / (NCH * 64 * (int)sizeof(T)) : LR_E_MAX;
}
template <class T, int NCH> constexpr int lr_c() { return LR_FILL_TEAMS * lr_e<T, NCH>(); }

template <class T, int NCH>
struct LrLds {
    T img[LR_BUFS][lr_c<T, NCH>()][NCH * 64];
    double g[LR_BUFS][lr_c<T, NCH>()], c[LR_BUFS][lr_c<T, NCH>()];
    double y[NCH * 64], y0[NCH * 64], q[NCH * 64], b[NCH * 64];      // y0: cg_base_part's own copy (team 0 alone)
    int32_t list[LR_S];
    int32_t cnt[LR_S / LR_THREADS][LR_THREADS / 64];
    int32_t go;
};

__device__ __forceinline__ void lds_piece(double *p, const double *d) { *(f64x2_t *)p = f64x2_t{d[0], d[1]}; }
__device__ __forceinline__ void lds_piece(float *p, const float *d) { *(f32x4_t *)p = f32x4_t{d[0], d[1], d[2], d[3]}; }

// One product and / or the right-hand side over a long row, by the whole workgroup.  y, q and b are team 0's registers;
// q leaves as MATVEC(y) (WANT_Q), b as rule C4's chain (WANT_B).  Every thread of the workgroup calls this, from one
// place: the two flags are workgroup-uniform values, not template arguments, so that the kernel holds one copy of the loop.
template <class T, bool WIDE, int NCH>
__device__ __forceinline__ void lr_product(LrLds<T, NCH> &s, const bool WANT_B, const bool WANT_Q, int64_t e0, int64_t e1, const int32_t *__restrict__ ci,
                                           const void *__restrict__ vals, int vt, bool scaled, int rhs_mode, const T *__restrict__ V,
                                           int64_t ldv, int k, const double *__restrict__ base, bool bwide, double rho,
                                           const double (&y)[NCH][4], double (&q)[NCH][4], double (&b)[NCH][4])
{
    constexpr int E = lr_e<T, NCH>(), C = lr_c<T, NCH>(), PIECE = 16 / (int)sizeof(T);
    const int tid = threadIdx.x, team = tid / CG_G, sub = tid % CG_G, wave = tid / 64, lane = tid % 64;
    if (WANT_Q && team == 0) {
#pragma unroll
        for (int c = 0; c < NCH; c++)
#pragma unroll
            for (int i = 0; i < 4; i++) s.y[64 * c + panel_off<T>(sub, i)] = y[c][i];
    }
    __syncthreads();                                                        // (and the last product's LDS reads are done)
    double yv[NCH][4], qc[NCH], bc[NCH];
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        qc[c] = 0.0, bc[c] = 0.0;
#pragma unroll
        for (int i = 0; i < 4; i++) yv[c][i] = 0.0;
    }
    if (wave == 0) {
        if (WANT_Q) {
            if (team == 0) {
                cg_head<T, NCH>(base, bwide, rho, k, sub, y, q, s.y0);
#pragma unroll
                for (int c = 0; c < NCH; c++)
#pragma unroll
                    for (int i = 0; i < 4; i++) s.q[64 * c + panel_off<T>(sub, i)] = q[c][i];
            }
            team_sync<64>();
#pragma unroll
            for (int c = 0; c < NCH; c++) qc[c] = s.q[64 * c + lane];
        }
    } else if (WANT_Q) {
#pragma unroll
        for (int c = 0; c < NCH; c++)
#pragma unroll
            for (int i = 0; i < 4; i++) yv[c][i] = s.y[64 * c + panel_off<T>(sub, i)];
    }

    const int64_t n = e1 - e0, last = e1 - 1, nchunks = (n + C - 1) / C;
    const int ft = team - 64 / CG_G;                                        // the fill team's number; below 0 in wavefront 0
    int32_t coln[E];                                                        // the next chunk's column indices
    if (wave != 0) {
#pragma unroll
        for (int x = 0; x < E; x++) coln[x] = ci[e0 + ft * E + x < last ? e0 + ft * E + x : last];
    }
    for (int64_t i = 0; i <= nchunks; i++) {
        if (wave != 0) {
            if (i < nchunks) {                                              // fill chunk i
                const int bf = (int)(i & 1);
                const int64_t eb = e0 + i * C + ft * E;
                T v[E][NCH][4];
                double wv[E], d[E];
#pragma unroll
                for (int x = 0; x < E; x++)                                 // (past the row: its last entry again, unused)
#pragma unroll
                    for (int c = 0; c < NCH; c++) panel_load4<T, WIDE>(V + (int64_t)coln[x] * ldv + 64 * c, sub, k - 64 * c, v[x][c]);
#pragma unroll
                for (int x = 0; x < E; x++) {
                    const int64_t e = eb + x < last ? eb + x : last;
                    wv[x] = vals ? csr_stored_val(vals, vt, e) : 1.0;
                    const int64_t en = eb + C + x < last ? eb + C + x : last;
                    coln[x] = ci[en];
                }
                if (WANT_Q) {
#pragma unroll
                    for (int x = 0; x < E; x++) d[x] = cg_dot<T, NCH>(v[x], yv, sub, k);
                }
#pragma unroll
                for (int x = 0; x < E; x++)
                    if (eb + x < e1) {
                        const int slot = ft * E + x;
#pragma unroll
                        for (int c = 0; c < NCH; c++)
#pragma unroll
                            for (int q0 = 0; q0 < 4; q0 += PIECE) lds_piece(&s.img[bf][slot][64 * c + panel_off<T>(sub, q0)], v[x][c] + q0);
                        if (sub == 0) {
                            if (WANT_Q) s.g[bf][slot] = scaled ? __dmul_rn(wv[x], d[x]) : d[x];
                            if (WANT_B)
                                s.c[bf][slot] = rhs_mode == CSRK_ALS_RHS_ONES ? 1.0
                                                                              : (rhs_mode == CSRK_ALS_RHS_VALUES ? wv[x] : __dadd_rn(1.0, wv[x]));
                        }
                    }
            }
        } else if (i >= 1) {                                                // chain chunk i - 1, storage order
            const int bf = (int)((i - 1) & 1);
            const int64_t left = n - (i - 1) * C;
            const int cnt = left < C ? (int)left : C;
#pragma unroll 4
            for (int sl = 0; sl < cnt; sl++) {
                const double g = WANT_Q ? s.g[bf][sl] : 0.0, cc = WANT_B ? s.c[bf][sl] : 0.0;
#pragma unroll
                for (int c = 0; c < NCH; c++) {
                    const double vv = (double)s.img[bf][sl][64 * c + lane];
                    if (WANT_Q) qc[c] = __builtin_fma(g, vv, qc[c]);
                    if (WANT_B) bc[c] = __builtin_fma(cc, vv, bc[c]);
                }
            }
        }
        __syncthreads();
    }

    if (wave == 0) {                                                        // back into team 0's layout
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            if (WANT_Q) s.q[64 * c + lane] = qc[c];
            if (WANT_B) s.b[64 * c + lane] = bc[c];
        }
        team_sync<64>();
        if (team == 0) {
#pragma unroll
            for (int c = 0; c < NCH; c++)
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int t = 64 * c + panel_off<T>(sub, i);
                    if (WANT_Q) q[c][i] = s.q[t];
                    if (WANT_B) b[c][i] = s.b[t];
                }
        }
    }
}

// Workgroup g lists the rows of [row_begin + g LR_S, row_begin + (g + 1) LR_S) with at least long_from entries, ascending,
// and solves them one after the other: als_cg_kernel's rules C4 - C7 with the walks replaced by lr_product.
template <class T, bool WIDE, int NCH>
__global__ __launch_bounds__(LR_THREADS) void als_cg_long_kernel(const void *__restrict__ rp, int ptr64, const int32_t *__restrict__ ci,
                                                                 const void *__restrict__ vals, int vt, int scaled, int32_t row_begin,
                                                                 int32_t row_end, const T *__restrict__ V, int64_t ldv, int32_t k,
                                                                 int rhs_mode, const double *__restrict__ base, int bwide, double lam,
                                                                 double lam_n, int32_t steps, double tol2, const double *x0, int64_t ldx0,
                                                                 double *out, int64_t ldo, double *__restrict__ resid,
                                                                 int32_t *__restrict__ taken_out, int64_t long_from,
                                                                 unsigned long long *__restrict__ census)
{
    __shared__ __attribute__((aligned(16))) LrLds<T, NCH> s;
    constexpr int PASSES = LR_S / LR_THREADS, WAVES = LR_THREADS / 64;
    const int tid = threadIdx.x, team = tid / CG_G, sub = tid % CG_G, wave = tid / 64, lane = tid % 64;
    const int64_t slice0 = (int64_t)row_begin + (int64_t)blockIdx.x * LR_S;

    uint64_t mask[PASSES];
#pragma unroll
    for (int ps = 0; ps < PASSES; ps++) {
        const int64_t row = slice0 + ps * LR_THREADS + tid;
        const bool is_long = row < row_end && load_ptr(rp, ptr64, row + 1) - load_ptr(rp, ptr64, row) >= long_from;
        mask[ps] = __ballot(is_long);
        if (lane == 0) s.cnt[ps][wave] = __popcll(mask[ps]);
    }
    __syncthreads();
    int n_long = 0;
#pragma unroll
    for (int ps = 0; ps < PASSES; ps++)
#pragma unroll
        for (int w = 0; w < WAVES; w++) {
            if (w == wave && ((mask[ps] >> lane) & 1)) s.list[n_long + __popcll(mask[ps] & ((1ull << lane) - 1))] = ps * LR_THREADS + tid;
            n_long += s.cnt[ps][w];
        }
    if (n_long == 0) return;                                                // (the whole workgroup)
    __syncthreads();

    for (int li = 0; li < n_long; li++) {
        const int64_t row = slice0 + s.list[li];
        const int64_t e0 = load_ptr(rp, ptr64, row), e1 = load_ptr(rp, ptr64, row + 1);
        const double rho = __builtin_fma(lam_n, (double)(e1 - e0), lam);
        double x[NCH][4], r[NCH][4], p[NCH][4], q[NCH][4];
#pragma unroll
        for (int c = 0; c < NCH; c++)
#pragma unroll
            for (int i = 0; i < 4; i++) x[c][i] = 0.0, r[c][i] = 0.0, p[c][i] = 0.0, q[c][i] = 0.0;

        if (x0 && team == 0) {                                              // (p carries x into the first product)
            const double *xr = x0 + (int64_t)(row - row_begin) * ldx0;
#pragma unroll
            for (int c = 0; c < NCH; c++)
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int t = 64 * c + panel_off<T>(sub, i);
                    x[c][i] = t < k ? xr[t] : 0.0;
                    p[c][i] = x[c][i];
                }
        }
        double rs = 0.0;
        int32_t taken = 0;
        // pass 0: rules C4 and C5 (b into r, and with an x0 q = MATVEC(x)); pass j >= 1: step j of rule C6.  The stop
        // decision is team 0's, published so that every loop stays workgroup-uniform.
        for (int pass = 0;; pass++) {
            if (pass > 0) {
                if (tid == 0) s.go = taken < steps && rs > tol2;
                __syncthreads();
                if (!s.go) break;
            }
            lr_product<T, WIDE, NCH>(s, pass == 0, pass > 0 || x0 != nullptr, e0, e1, ci, vals, vt, scaled != 0, rhs_mode, V, ldv, k, base,
                                     bwide != 0, rho, p, q, r);
            if (team == 0) {
                if (pass == 0) {
#pragma unroll
                    for (int c = 0; c < NCH; c++)
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            if (x0) r[c][i] = __dsub_rn(r[c][i], q[c][i]);
                            p[c][i] = r[c][i];
                        }
                    rs = cg_dot<T, NCH>(r, r, sub, k);
                } else {
                    const double pq = cg_dot<T, NCH>(p, q, sub, k);
                    const double alpha = __ddiv_rn(rs, pq);
#pragma unroll
                    for (int c = 0; c < NCH; c++)
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            x[c][i] = __builtin_fma(alpha, p[c][i], x[c][i]);
                            r[c][i] = __builtin_fma(-alpha, q[c][i], r[c][i]);
                        }
                    const double rn = cg_dot<T, NCH>(r, r, sub, k);
                    const double beta = __ddiv_rn(rn, rs);
#pragma unroll
                    for (int c = 0; c < NCH; c++)
#pragma unroll
                        for (int i = 0; i < 4; i++) p[c][i] = __builtin_fma(beta, p[c][i], r[c][i]);
                    rs = rn;
                }
            }
            taken += pass > 0;
        }

        if (team == 0) {
            double *o = out + (int64_t)(row - row_begin) * ldo;
#pragma unroll
            for (int c = 0; c < NCH; c++)
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int t = 64 * c + panel_off<T>(sub, i);
                    if (t < k) o[t] = x[c][i];
                }
            if (sub == 0) {
                if (resid) resid[row - row_begin] = rs;
                if (taken_out) taken_out[row - row_begin] = taken;
                if (census) {
                    atomicAdd(census, 1ull);
                    atomicAdd(census + 1, (unsigned long long)(e1 - e0));
                }
            }
        }
    }
}

// what can be refused without looking at the handle (the entries do, before they look: these need no device)
static int cg_check_scalars(int32_t row_begin, int32_t row_end, int64_t ldv, int32_t k, int panel_type, int scale, int rhs_mode,
                            int32_t steps, double tol2, bool has_x0, int64_t ldx0, int64_t ldo)
{
    CSRK_CHECK_K("", k);
    CSRK_CHECK_ONE_PANEL(k, ldv);
    CSRK_REQUIRE(ldo >= k, "bad output geometry k=%d ldo=%lld", k, (long long)ldo);
    CSRK_CHECK_PANEL_TYPE("", panel_type);
    CSRK_CHECK_SCALE(scale);
    CSRK_REQUIRE(rhs_mode == CSRK_ALS_RHS_ONES || rhs_mode == CSRK_ALS_RHS_VALUES || rhs_mode == CSRK_ALS_RHS_ONE_PLUS,
                 "rhs_mode must be CSRK_ALS_RHS_ONES, _VALUES or _ONE_PLUS, not %d", rhs_mode);
    CSRK_REQUIRE(steps >= 0, "steps must not be negative (steps=%d)", steps);
    CSRK_REQUIRE(tol2 >= 0.0, "tol2 must be a number that is not negative (tol2=%g)", tol2);      // (false for NaN)
    CSRK_REQUIRE(!has_x0 || ldx0 >= k, "bad x0 geometry k=%d ldx0=%lld", k, (long long)ldx0);
    CSRK_CHECK_ROW_ORDER("", row_begin, row_end);
    if (k > CG_K_MAX) {
        set_error("csrk_als_rows_cg: k=%d is above the largest supported k=%d (csrk_als_cg_limits)", k, CG_K_MAX);
        return CSRK_ERR_UNSUPPORTED;
    }
    return CSRK_OK;
}

static int cg_check(Matrix *m, int32_t row_begin, int32_t row_end, int64_t ldv, int32_t k, int panel_type, int scale, int rhs_mode,
                    int32_t steps, double tol2, bool has_x0, int64_t ldx0, int64_t ldo)
{
    CSRK_TRY(cg_check_scalars(row_begin, row_end, ldv, k, panel_type, scale, rhs_mode, steps, tol2, has_x0, ldx0, ldo));
    CSRK_CHECK_ROW_RANGE("", row_begin, row_end, m->nrows);
    return CSRK_OK;
}

// ---- the long-row switch and the calling thread's census (rule C11) ----
static std::atomic<int64_t> g_cg_long{-1};      // -1: follow CSRK_ALS_CG_LONG; 0: off; >= 1: a row of that many entries is long
static thread_local int64_t t_cg_stats[6];

// the L in force: 0 = the class is off
static int64_t cg_long_in_force()
{
    const int64_t v = g_cg_long.load();
    if (v >= 0) return v;
    const char *e = getenv("CSRK_ALS_CG_LONG");
    if (!e || !*e) return LR_DEFAULT_LONG;
    char *end = nullptr;
    const long long x = strtoll(e, &end, 10);
    return (end == e || *end || x < 0) ? LR_DEFAULT_LONG : (int64_t)x;      // (not a decimal count: the default)
}

static void cg_stats_clear()
{
    for (int64_t &v : t_cg_stats) v = 0;
}

// census: two device counters (rows, entries) the long-row kernel adds to, or NULL
static int cg_device(Matrix *m, int32_t row_begin, int32_t row_end, const void *dV, int64_t ldv, int32_t k, int panel_type, int scale,
                     int rhs_mode, const double *dbase, double lam, double lam_n, int32_t steps, double tol2, const double *dx0,
                     int64_t ldx0, double *dout, int64_t ldo, double *dresid, int32_t *dtaken, hipStream_t s,
                     unsigned long long *census)
{
    CSRK_TRY(cg_check(m, row_begin, row_end, ldv, k, panel_type, scale, rhs_mode, steps, tol2, dx0 != nullptr, ldx0, ldo));
    const int64_t L = cg_long_in_force();
    t_cg_stats[1] = L;
    if (row_begin == row_end) return CSRK_OK;
    CSRK_REQUIRE(dout && (dV || m->nnz == 0), "V or out is NULL");
    const size_t es = panel_es(panel_type);
    CSRK_REQUIRE(((uintptr_t)dV % es) == 0 && ((uintptr_t)dout % 8) == 0 && ((uintptr_t)dbase % 8) == 0 && ((uintptr_t)dx0 % 8) == 0 &&
                     ((uintptr_t)dresid % 8) == 0 && ((uintptr_t)dtaken % 4) == 0,
                 "V, base, x0, out, resid or taken is not aligned to its element size");
    mark_user_stream(m, s);
    const bool wide = panel_16b(dV, ldv, es);      // a lane loads four columns at a time, as csrk_sddmm's do: no k term
    const int bwide = dbase && panel_16b(dbase, k, 8);
    const bool stored = m->val_type != CSRK_VAL_NONE;               // (a structure-only matrix: every value is 1.0)
    const int scaled = scale && stored;
    const void *vals = stored && (scaled || rhs_mode != CSRK_ALS_RHS_ONES) ? m->d_values : nullptr;
    const int64_t n = (int64_t)row_end - row_begin;
    const unsigned grid = (unsigned)ceil_div(n, CG_TEAMS);
    // the long rows first, one workgroup per LR_S rows of the range (a matrix without entries has none); then the teams,
    // which leave those rows alone.  Class off: a length no row reaches, and the one launch is the whole call.
    const bool go_long = L > 0 && m->nnz > 0;
    const unsigned grid_long = (unsigned)ceil_div(n, LR_S);
    const int64_t long_from = L > 0 ? L : INT64_MAX;
#define CG_ARGS(T)                                                                                                                \
    m->d_rowptrs, m->ptr64, m->d_colinds, vals, m->val_type, scaled, row_begin, row_end, (const T *)dV, ldv, k, rhs_mode, dbase, bwide, \
        lam, lam_n, steps, tol2, dx0, ldx0, dout, ldo, dresid, dtaken, long_from
#define CG_GO(T, W, NCH)                                                                                                          \
    do {                                                                                                                          \
        if (go_long) als_cg_long_kernel<T, W, NCH><<<grid_long, LR_THREADS, 0, s>>>(CG_ARGS(T), census);                          \
        als_cg_kernel<T, W, NCH><<<grid, CG_THREADS, 0, s>>>(CG_ARGS(T));                                                         \
    } while (0)
#define CG_NCH(T, W)                                                                                                              \
    do {                                                                                                                          \
        if (k <= 64) CG_GO(T, W, 1);                                                                                              \
        else CG_GO(T, W, 2);                                                                                                      \
    } while (0)
    if (panel_type == CSRK_VAL_F64) {
        if (wide) CG_NCH(double, true);
        else CG_NCH(double, false);
    } else {
        if (wide) CG_NCH(float, true);
        else CG_NCH(float, false);
    }
#undef CG_NCH
#undef CG_GO
#undef CG_ARGS
    CSRK_LAUNCH_CHECK();
    t_cg_stats[0] = 1;
    t_cg_stats[2] = go_long;
    t_cg_stats[3] = go_long ? grid_long : 0;
    t_cg_stats[4] = t_cg_stats[5] = go_long ? -1 : 0;               // (the host form replaces these by the kernel's counts)
    return CSRK_OK;
}

}  // namespace csrk

using namespace csrk;

extern "C" {

int csrk_als_cg_limits(int64_t *out, int n)
{
    CSRK_REQUIRE(out && n >= 0, "csrk_als_cg_limits: out is NULL or n < 0");
    const int64_t v[3] = {CG_K_MAX, CG_G, CG_E};
    for (int i = 0; i < n && i < 3; i++) out[i] = v[i];
    return CSRK_OK;
}

int csrk_als_cg_long_limits(int64_t *out, int n)
{
    CSRK_REQUIRE(out && n >= 0, "csrk_als_cg_long_limits: out is NULL or n < 0");
    const int64_t v[8] = {LR_DEFAULT_LONG, LR_THREADS, LR_S, lr_c<double, 1>(), lr_c<double, 2>(), lr_c<float, 1>(), lr_c<float, 2>(),
                          LR_BUFS};
    for (int i = 0; i < n && i < 8; i++) out[i] = v[i];
    return CSRK_OK;
}

int csrk_als_cg_set_long(int64_t entries)
{
    CSRK_REQUIRE(entries >= -1, "entries must be -1 (environment), 0 (off) or a count of at least 1, not %lld", (long long)entries);
    g_cg_long.store(entries);
    return CSRK_OK;
}

int csrk_als_cg_get_long(int64_t *entries)
{
    CSRK_REQUIRE(entries, "entries is NULL");
    *entries = cg_long_in_force();
    return CSRK_OK;
}

int csrk_als_cg_last_stats(int64_t *out, int n)
{
    CSRK_REQUIRE(out && n >= 0, "csrk_als_cg_last_stats: out is NULL or n < 0");
    for (int i = 0; i < n && i < 6; i++) out[i] = t_cg_stats[i];
    return CSRK_OK;
}

int csrk_als_rows_cg_device(csrk_handle_t h, int32_t row_begin, int32_t row_end, const void *d_V, int64_t ldv, int32_t k,
                            int panel_type, int scale, int rhs_mode, const double *d_base, double lam, double lam_n, int32_t steps,
                            double tol2, const double *d_x0, int64_t ldx0, double *d_out, int64_t ldo, double *d_resid,
                            int32_t *d_taken, void *stream)
{
    cg_stats_clear();
    CSRK_TRY(cg_check_scalars(row_begin, row_end, ldv, k, panel_type, scale, rhs_mode, steps, tol2, d_x0 != nullptr, ldx0, ldo));
    Matrix *m = from_handle(h);
    if (!m) return CSRK_ERR_INVALID;
    const int rc = cg_device(m, row_begin, row_end, d_V, ldv, k, panel_type, scale, rhs_mode, d_base, lam, lam_n, steps, tol2, d_x0, ldx0,
                             d_out, ldo, d_resid, d_taken, (hipStream_t)stream, nullptr);
    if (rc != CSRK_OK) cg_stats_clear();
    return rc;
}

// the host form's work; csrk_als_rows_cg clears the census when this refuses or fails
static int cg_host(csrk_handle_t h, int32_t row_begin, int32_t row_end, const void *V, int64_t ldv, int32_t k, int panel_type, int scale,
                   int rhs_mode, const double *base, double lam, double lam_n, int32_t steps, double tol2, const double *x0, int64_t ldx0,
                   double *out, int64_t ldo, double *resid, int32_t *taken)
{
    CSRK_TRY(cg_check_scalars(row_begin, row_end, ldv, k, panel_type, scale, rhs_mode, steps, tol2, x0 != nullptr, ldx0, ldo));
    Matrix *m = from_handle(h);
    if (!m) return CSRK_ERR_INVALID;
    // argument checks first, with the caller's pointers (the device call below sees packed copies)
    CSRK_TRY(cg_check(m, row_begin, row_end, ldv, k, panel_type, scale, rhs_mode, steps, tol2, x0 != nullptr, ldx0, ldo));
    if (row_begin == row_end) {
        t_cg_stats[1] = cg_long_in_force();
        return CSRK_OK;
    }
    CSRK_REQUIRE(out && (V || m->nnz == 0), "V or out is NULL");
    const size_t n = (size_t)(row_end - row_begin);
    DevBuf dV, dB, dX, dO, dR, dT, dC;
    CSRK_TRY(pack_panel(dV, V, ldv, k, panel_es(panel_type), m->ncols));
    CSRK_TRY(dO.alloc(n * k * 8));
    CSRK_TRY(dR.alloc(n * 8));
    CSRK_TRY(dT.alloc(n * 4));
    CSRK_TRY(dC.alloc(16));
    CSRK_HIP(hipMemsetAsync(dC.p, 0, 16, nullptr));
    if (base) {
        CSRK_TRY(dB.alloc((size_t)k * k * 8));
        CSRK_HIP(hipMemcpy(dB.p, base, (size_t)k * k * 8, hipMemcpyHostToDevice));
    }
    if (x0) CSRK_TRY(pack_panel(dX, x0, ldx0, k, 8, (int64_t)n));
    CSRK_TRY(cg_device(m, row_begin, row_end, dV.p, k, k, panel_type, scale, rhs_mode, base ? dB.as<double>() : nullptr, lam, lam_n,
                       steps, tol2, x0 ? dX.as<double>() : nullptr, k, dO.as<double>(), k, dR.as<double>(), dT.as<int32_t>(), nullptr,
                       dC.as<unsigned long long>()));
    CSRK_TRY(unpack_panel(out, ldo, dO, k, 8, (int64_t)n));
    if (resid) CSRK_HIP(hipMemcpy(resid, dR.p, n * 8, hipMemcpyDeviceToHost));
    if (taken) CSRK_HIP(hipMemcpy(taken, dT.p, n * 4, hipMemcpyDeviceToHost));
    unsigned long long counts[2];
    CSRK_HIP(hipMemcpy(counts, dC.p, 16, hipMemcpyDeviceToHost));
    t_cg_stats[4] = (int64_t)counts[0], t_cg_stats[5] = (int64_t)counts[1];
    return CSRK_OK;
}

int csrk_als_rows_cg(csrk_handle_t h, int32_t row_begin, int32_t row_end, const void *V, int64_t ldv, int32_t k, int panel_type,
                     int scale, int rhs_mode, const double *base, double lam, double lam_n, int32_t steps, double tol2,
                     const double *x0, int64_t ldx0, double *out, int64_t ldo, double *resid, int32_t *taken)
{
    cg_stats_clear();
    const int rc = cg_host(h, row_begin, row_end, V, ldv, k, panel_type, scale, rhs_mode, base, lam, lam_n, steps, tol2, x0, ldx0, out,
                           ldo, resid, taken);
    if (rc != CSRK_OK) cg_stats_clear();
    return rc;
}

}  // extern "C"
