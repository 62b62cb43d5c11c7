// linsolver.hip -- gfx950 kernels for the block-ILU0 / BiCGStab solve (see linsolver.hpp).
//
// All kernels are HBM-bandwidth bound (<= 0.25 flop/byte): no MFMA.  One thread owns one block row;
// the SELL-64 layout makes every matrix / index load of a wavefront one contiguous segment, the
// vectors are component-major planes so x[col] gathers of neighbouring rows coalesce as well.
//
// Reductions are order-deterministic and need no extra launches: a producer kernel writes one
// partial per workgroup, every workgroup of the consumer kernel re-reduces the (<= 1024-entry)
// partial array in the same fixed order and derives the BiCGStab scalars itself.  A device-resident
// `done` flag lets the host enqueue iterations ahead of the convergence result (no per-iteration
// host synchronisation); the host polls a host-mapped control block after an event.
#include "linsolver.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <type_traits>

namespace opmgpu {

int xcd_mode()
{
    static const int m = env_int("OPMGPU_XCD", 1);
    return m;
}

constexpr int kMaxPart = 1024;      // workgroups (= partials) of every reducing kernel
constexpr int kBndPart = 256;       // + those of the second (cut-adjacent rows) SpMV launch when the halo exchange is overlapped
constexpr int kCsRowParts = 8192;   // ... of the fused CPR row pass (one row per thread up to 2M rows: latency-bound, wants occupancy)

// ------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ long vidx(int base_slot, int lane) { return long(base_slot) * 576 + lane; }

// fixed-order sum of NV partial arrays of n entries; result broadcast to all threads of the block
template <int NV>
__device__ __forceinline__ void reduce_partials(const double* const (&arr)[NV], int n, double (&out)[NV], double* sm /* >= 4*NV + NV */)
{
    double acc[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        acc[k] = 0.0;
        for (int i = threadIdx.x; i < n; i += kBlock) acc[k] += arr[k][i];
    }
    block_sum<NV>(acc, sm);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) sm[4 * NV + k] = acc[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) out[k] = sm[4 * NV + k];
    __syncthreads();
}

// y = A x  (+ fused dot products: NDOT==1: <w1,y>; NDOT==2: <y,w1>, <y,y>)
// MatrixAdapter::apply + the scalar products of BiCGSTABSolver::apply.  Grid-stride over 256-row
// chunks so that a reducing launch has at most kMaxPart workgroups.  mask (multi-GPU): rows that are
// not owned produce 0.
//
// pin != nullptr (single GPU, x = M^-1 pin where the last stage of M^-1 is the ILU0 of THIS matrix): for the n0
// level-0 rows the product is known in closed form.  Such a row has no lower entries, so U_ij = A_ij and
// Dinv_i = A_ii^-1; with x = c + ILU0^-1 z  (ILU0 alone: c = 0, z = pin;  CPR: c = [x_p;0;0], z = pin - A c)
//   (ILU0^-1 z)_i = A_ii^-1 (w z_i - sum_j A_ij (ILU0^-1 z)_j)  =>  (A ILU0^-1 z)_i = w z_i
//   (A x)_i = (A c)_i + w z_i = (pin_i - z_i) + w z_i = pin_i - (1 - w) z_i .
// Those rows (half of all rows with the 2-colour ordering) need no matrix traffic.  Light and heavy rows
// are chunked separately so that every XCD gets the same share of both.
//
// GM == 1 (left-preconditioned GMRES, relaxation 1, see gmres()): x is a basis vector v_i, not M^-1 of a vector in memory.  On a
// level-0 row A M^-1 is the identity (the formula above with w = 1), so by induction over the Arnoldi recurrence
//   v_0 = M^-1 b / beta,   v_{i+1} = (M^-1 A v_i - sum_{k<=i} h_ki v_k) / h_{i+1,i}
// every product is a multiple of the cycle's base vector there: (A v_i)_row = gamma_i base_row (base = b, after a restart the true
// defect).  pin = base, *gamma = gamma_i (device-resident, k_gm_normalize / k_gm_givens advance it).  A perforated level-0 row is no
// such row (the well operator adds P_i t_w): lightmask[row] == 0 sends it through the full row product.
// y_i += P_i t_w on a perforated row (t_w = Q_w x from k_lowrank_reduce)
template <class S>
__device__ __forceinline__ void lowrank_add(const LowRankOp& lr, int row, S& y0, S& y1, S& y2)
{
    // a row of several wells: one term per perforation, in ascending perforation index
    const int pf = lr.perf_of_row[row];
    if (pf < 0) return;
    {
        const double* __restrict__ P = lr.P + 21 * long(pf);
        const double* __restrict__ t = lr.t + 7 * lr.perf_well[pf];
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        // the 28 operands in two batches (same sums, same order): all at once they are the kernel's register peak -- 56 VGPRs for a handful of
        // rows -- and cost every row a wave of occupancy
#pragma unroll
        for (int k = 0; k < 4; ++k) { a0 += P[k] * t[k]; a1 += P[7 + k] * t[k]; a2 += P[14 + k] * t[k]; }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 4; k < 7; ++k) { a0 += P[k] * t[k]; a1 += P[7 + k] * t[k]; a2 += P[14 + k] * t[k]; }
        y0 += S(a0); y1 += S(a1); y2 += S(a2);
    }
    // the further perforations of a row of several wells (a handful of rows per deck), same sums in the same order; rolled, so that the rows
    // of one perforation or none keep the kernel's registers
#pragma nounroll
    for (int nx = lr.perf_next[pf]; nx >= 0; nx = lr.perf_next[nx]) {
        const double* __restrict__ P = lr.P + 21 * long(nx);
        const double* __restrict__ t = lr.t + 7 * lr.perf_well[nx];
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma nounroll
        for (int k = 0; k < 7; ++k) { a0 += P[k] * t[k]; a1 += P[7 + k] * t[k]; a2 += P[14 + k] * t[k]; }
        y0 += S(a0); y1 += S(a1); y2 += S(a2);
    }
}
// t_w = Q_w x: one workgroup per well, fixed reduction order
template <class S>
__global__ __launch_bounds__(kBlock) void k_lowrank_reduce(LowRankOp lr, int nbp, const S* __restrict__ x, const SolveCtl* __restrict__ ctl)
{
    __shared__ double sm[28];
    if (ctl && ctl->done) return;
    const int w = blockIdx.x;
    double acc[7] = { 0, 0, 0, 0, 0, 0, 0 };
    for (int j = lr.connpos[w] + threadIdx.x; j < lr.connpos[w + 1]; j += kBlock) {
        const int row = lr.perf_row[j];
        const double x0 = double(x[row]), x1 = double(x[nbp + row]), x2 = double(x[2 * long(nbp) + row]);
        const double* __restrict__ Q = lr.Q + 21 * long(j);
#pragma unroll
        for (int k = 0; k < 7; ++k) acc[k] += Q[3 * k] * x0 + Q[3 * k + 1] * x1 + Q[3 * k + 2] * x2;
    }
    block_sum<7>(acc, sm);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 7; ++k) lr.t[7 * w + k] = acc[k];
    }
}

// multi-GPU: rows whose closed form survives the halo exchange = owned rows with only owned neighbours
__global__ __launch_bounds__(kBlock) void k_light_mask(int nb, const int32_t* __restrict__ slice_ptr, const int32_t* __restrict__ col,
                                                       const int16_t* __restrict__ rowlen, const int8_t* __restrict__ owner, int8_t* __restrict__ ok)
{
    const int row = blockIdx.x * kBlock + threadIdx.x;
    if (row >= nb) return;
    const int base = slice_ptr[row >> 6], lane = row & 63;
    bool good = owner[row] != 0;
    for (int k = 0, len = rowlen[row]; k < len; ++k) good = good && owner[col[long(base + k) * 64 + lane]] != 0;
    ok[row] = good ? 1 : 0;
}

// GMRES closed form: level-0 rows that keep it = those without a perforation (1), the others take the full row product (0)
__global__ __launch_bounds__(kBlock) void k_unperforated_mask(int n, const int32_t* __restrict__ perf_of_row, int8_t* __restrict__ ok)
{
    const int row = blockIdx.x * kBlock + threadIdx.x;
    if (row < n) ok[row] = perf_of_row[row] < 0 ? 1 : 0;
}

template <class S, int NDOT, int GM = 0>
__global__ __launch_bounds__(kBlock) void k_spmv(int xm, int nb, int nbp, const int32_t* __restrict__ slice_ptr,
                                                 const int32_t* __restrict__ col, const S* __restrict__ val,
                                                 const S* __restrict__ x, S* __restrict__ y,
                                                 const S* __restrict__ w1, const int8_t* __restrict__ mask,
                                                 const SolveCtl* __restrict__ ctl, double* __restrict__ p0, double* __restrict__ p1,
                                                 const S* __restrict__ pin, const S* __restrict__ zin, int n0, S w, LowRankOp lr,
                                                 const int8_t* __restrict__ lightmask, int phase = 0, const int8_t* __restrict__ interior = nullptr,
                                                 const double* __restrict__ gamma = nullptr)
{
    // phase (multi-GPU, halo exchange in flight): 1 = only the rows of `interior` (owned, no ghost neighbour: they read no halo value),
    // 2 = only the others; 0 = all rows.  The partials of the two launches are laid side by side by the caller.
    __shared__ double sm[8];
    if (ctl && ctl->done) return;
    double acc[2] = { 0.0, 0.0 };
    const int nlight = pin ? n0 : 0;
    {
        const int nchunks = (nlight + kBlock - 1) / kBlock;
        for (int ch = xcd_first(nchunks, xm); ch < xcd_end(nchunks, xm); ch += xcd_stride(xm)) {
            const int row = ch * kBlock + threadIdx.x;
            if (row >= nlight) continue;
            if (phase && (phase == 1) != (interior[row] != 0)) continue;
            S y0, y1, y2;
            if (!lightmask || lightmask[row]) {
                if (GM) {
                    const S g = S(*gamma);
                    y0 = g * pin[row]; y1 = g * pin[nbp + row]; y2 = g * pin[2 * nbp + row];
                } else {
                    const S om = S(1) - w;
                    y0 = pin[row] - om * zin[row]; y1 = pin[nbp + row] - om * zin[nbp + row]; y2 = pin[2 * nbp + row] - om * zin[2 * nbp + row];
                }
            } else {
                // multi-GPU: a level-0 row next to a ghost cell (its x was replaced by the owner's value) or a ghost row itself;
                // GMRES: a perforated level-0 row
                y0 = 0; y1 = 0; y2 = 0;
                if (!mask || mask[row]) {
                    const int sl = row >> 6, lane = row & 63;
                    const int base = slice_ptr[sl], width = slice_ptr[sl + 1] - base;
                    const S* __restrict__ v = val + vidx(base, lane);
                    const int32_t* __restrict__ c = col + long(base) * 64 + lane;
                    for (int k = 0; k < width; ++k) {
                        const int cc = c[k * 64];
                        const S x0 = x[cc], x1 = x[nbp + cc], x2 = x[2 * nbp + cc];
                        const S* __restrict__ b = v + k * 576;
                        y0 += b[0] * x0 + b[64] * x1 + b[128] * x2;
                        y1 += b[192] * x0 + b[256] * x1 + b[320] * x2;
                        y2 += b[384] * x0 + b[448] * x1 + b[512] * x2;
                    }
                }
            }
            if (lr.perf_of_row) lowrank_add(lr, row, y0, y1, y2);
            y[row] = y0; y[nbp + row] = y1; y[2 * nbp + row] = y2;
            if (NDOT >= 1) acc[0] += double(w1[row]) * double(y0) + double(w1[nbp + row]) * double(y1) + double(w1[2 * nbp + row]) * double(y2);
            if (NDOT == 2) acc[1] += double(y0) * double(y0) + double(y1) * double(y1) + double(y2) * double(y2);
        }
    }
    const int nchunks = (nb - nlight + kBlock - 1) / kBlock;
    for (int ch = xcd_first(nchunks, xm); ch < xcd_end(nchunks, xm); ch += xcd_stride(xm)) {
        const int row = nlight + ch * kBlock + threadIdx.x;
        if (row >= nb) continue;
        if (phase && (phase == 1) != (interior[row] != 0)) continue;
        const int sl = row >> 6, lane = row & 63;
        const int base = slice_ptr[sl], width = slice_ptr[sl + 1] - base;
        const S* __restrict__ v = val + vidx(base, lane);
        const int32_t* __restrict__ c = col + long(base) * 64 + lane;
        S y0 = 0, y1 = 0, y2 = 0;
        if (!mask || mask[row]) {
            for (int k = 0; k < width; ++k) {
                const int cc = c[k * 64];
                const S x0 = x[cc], x1 = x[nbp + cc], x2 = x[2 * nbp + cc];
                const S* __restrict__ b = v + k * 576;
                y0 += b[0] * x0 + b[64] * x1 + b[128] * x2;
                y1 += b[192] * x0 + b[256] * x1 + b[320] * x2;
                y2 += b[384] * x0 + b[448] * x1 + b[512] * x2;
            }
        }
        if (lr.perf_of_row) lowrank_add(lr, row, y0, y1, y2);
        y[row] = y0; y[nbp + row] = y1; y[2 * nbp + row] = y2;
        if (NDOT >= 1) acc[0] += double(w1[row]) * double(y0) + double(w1[nbp + row]) * double(y1) + double(w1[2 * nbp + row]) * double(y2);
        if (NDOT == 2) acc[1] += double(y0) * double(y0) + double(y1) * double(y1) + double(y2) * double(y2);
    }
    if (NDOT >= 1) {
        block_sum<2>(acc, sm);
        if (threadIdx.x == 0) {
            p0[blockIdx.x] = acc[0];
            if (NDOT == 2) p1[blockIdx.x] = acc[1];
        }
    }
}

// forward sweep of one level l >= 1: v_i = w d_i - sum_{j lower} L_ij y_j with y_j = w d_j for level-0
// rows (their forward sweep is the identity, so it is never launched) and y_j = v_j otherwise.  For the
// top level the pivot inverse is applied at once (no upper entries there).
// ParallelOverlappingILU0::apply, lower part; the relaxation factor w is folded in (the sweeps are linear).
// FP (LinSolver::cpr_factor_p; the top level of a two-level plan, w = 1, xp given): the row forms its own right-hand side.  d is the CPR
// application's input, A the unfactorised matrix, s holds on the level-0 rows their stage-2 residual without its diagonal term
// (k_cpr_presidual_l0).  The row starts from d_i - A_ii[:,0] x_p,i and reads s_r where the plain form reads w d_r: L_ir = A_ir A_rr^-1
// carries A_ir[:,0] x_p,r, the part of the row's residual that was left out of s_r, into the sum.
template <class S, bool FP = false>
__global__ __launch_bounds__(kBlock) void k_ilu_lower(int xm, int lo, int hi, int n0, int nbp, int top, S w, const int32_t* __restrict__ slice_ptr,
                                                      const int32_t* __restrict__ col, const int16_t* __restrict__ nlower,
                                                      const S* __restrict__ lu, const S* __restrict__ d, S* __restrict__ v,
                                                      const SolveCtl* __restrict__ ctl, const S* __restrict__ xp = nullptr,
                                                      const S* __restrict__ A = nullptr, const S* __restrict__ s = nullptr)
{
    if (ctl && ctl->done) return;
    const int nchunks = (hi - lo + kBlock - 1) / kBlock;
    const int ch = xcd_first(nchunks, xm);
    if (ch >= xcd_end(nchunks, xm)) return;
    const int row = lo + ch * kBlock + threadIdx.x;
    if (row >= hi) return;
    const int base = slice_ptr[row >> 6], lane = row & 63, nl = nlower[row];
    const S* __restrict__ m = lu + vidx(base, lane);
    const int32_t* __restrict__ c = col + long(base) * 64 + lane;
    S r0, r1, r2;
    if constexpr (FP) {
        const S* __restrict__ a = A + vidx(base, lane) + nl * 576;       // A's own diagonal block: its pressure column
        const S xi = xp[row];
        r0 = d[row] - a[0] * xi; r1 = d[nbp + row] - a[192] * xi; r2 = d[2 * nbp + row] - a[384] * xi;
    } else { r0 = w * d[row]; r1 = w * d[nbp + row]; r2 = w * d[2 * nbp + row]; }
    for (int k = 0; k < nl; ++k) {
        const int cc = c[k * 64];
        S x0, x1, x2;
        if constexpr (FP) { x0 = s[cc]; x1 = s[nbp + cc]; x2 = s[2 * nbp + cc]; }          // (every lower entry lies on level 0)
        else if (cc < n0) { x0 = w * d[cc]; x1 = w * d[nbp + cc]; x2 = w * d[2 * nbp + cc]; }
        else { x0 = v[cc]; x1 = v[nbp + cc]; x2 = v[2 * nbp + cc]; }
        const S* __restrict__ b = m + k * 576;
        r0 -= b[0] * x0 + b[64] * x1 + b[128] * x2;
        r1 -= b[192] * x0 + b[256] * x1 + b[320] * x2;
        r2 -= b[384] * x0 + b[448] * x1 + b[512] * x2;
    }
    if (top) {
        const S* __restrict__ b = m + nl * 576;
        const S t0 = b[0] * r0 + b[64] * r1 + b[128] * r2;
        const S t1 = b[192] * r0 + b[256] * r1 + b[320] * r2;
        const S t2 = b[384] * r0 + b[448] * r1 + b[512] * r2;
        r0 = t0; r1 = t1; r2 = t2;
        if (xp) r0 += xp[row];      // CPR, top level of a two-level plan: the row is final, the pressure correction is added here (LinSolver::cpr_cancel_p)
    }
    v[row] = r0; v[nbp + row] = r1; v[2 * nbp + row] = r2;
}

// backward sweep of one level: v_i = Dinv_i (y_i - sum_{j upper} U_ij v_j), y_i = w d_i on level 0
template <class S>
__global__ __launch_bounds__(kBlock) void k_ilu_upper(int xm, int lo, int hi, int n0, int nbp, S w, const int32_t* __restrict__ slice_ptr,
                                                      const int32_t* __restrict__ col, const int16_t* __restrict__ nlower,
                                                      const int16_t* __restrict__ rowlen, const S* __restrict__ lu,
                                                      const S* __restrict__ d, S* __restrict__ v, const SolveCtl* __restrict__ ctl,
                                                      const int8_t* __restrict__ simple, const S* __restrict__ A)
{
    if (ctl && ctl->done) return;
    const int nchunks = (hi - lo + kBlock - 1) / kBlock;
    const int ch = xcd_first(nchunks, xm);
    if (ch >= xcd_end(nchunks, xm)) return;
    const int row = lo + ch * kBlock + threadIdx.x;
    if (row >= hi) return;
    const int base = slice_ptr[row >> 6], lane = row & 63, nl = nlower[row], len = rowlen[row];
    // U entries of a "simple" row (all its ILU0 updates hit the diagonal block) are the entries of the factorised matrix itself: the
    // factorisation does not copy them (k_ilu_factor), they are read from A -- which the SpMV keeps warm in the Infinity Cache anyway
    const S* __restrict__ m = lu + vidx(base, lane);
    const S* __restrict__ mu = (simple[row] ? A : lu) + vidx(base, lane);
    const int32_t* __restrict__ c = col + long(base) * 64 + lane;
    S r0, r1, r2;
    if (row < n0) { r0 = w * d[row]; r1 = w * d[nbp + row]; r2 = w * d[2 * nbp + row]; }
    else { r0 = v[row]; r1 = v[nbp + row]; r2 = v[2 * nbp + row]; }
    for (int k = nl + 1; k < len; ++k) {
        const int cc = c[k * 64];
        const S x0 = v[cc], x1 = v[nbp + cc], x2 = v[2 * nbp + cc];
        const S* __restrict__ b = mu + k * 576;
        r0 -= b[0] * x0 + b[64] * x1 + b[128] * x2;
        r1 -= b[192] * x0 + b[256] * x1 + b[320] * x2;
        r2 -= b[384] * x0 + b[448] * x1 + b[512] * x2;
    }
    const S* __restrict__ b = m + nl * 576;
    v[row] = b[0] * r0 + b[64] * r1 + b[128] * r2;
    v[nbp + row] = b[192] * r0 + b[256] * r1 + b[320] * r2;
    v[2 * nbp + row] = b[384] * r0 + b[448] * r1 + b[512] * r2;
}

template <class S> __device__ __forceinline__ void ld9(const S* __restrict__ a, int32_t e, S (&m)[9])
{
    const S* p = a + long(e >> 6) * 576 + (e & 63);
#pragma unroll
    for (int q = 0; q < 9; ++q) m[q] = p[q * 64];
}
template <class S> __device__ __forceinline__ void st9(S* __restrict__ a, int32_t e, const S (&m)[9])
{
    S* p = a + long(e >> 6) * 576 + (e & 63);
#pragma unroll
    for (int q = 0; q < 9; ++q) p[q * 64] = m[q];
}
template <class S> __device__ __forceinline__ void mm9(const S (&a)[9], const S (&b)[9], S (&c)[9])
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

// numeric block-ILU(0) of the rows of one level (IKJ; dune-istl bilu0_decomposition order inside a
// row; pivots inverted explicitly with the cofactor formula like opm-simulators' MatrixBlock).
template <class S>
__global__ __launch_bounds__(kBlock) void k_ilu_factor(int lo, int hi, const int32_t* __restrict__ slice_ptr, const int32_t* __restrict__ col,
                                                       const int16_t* __restrict__ nlower, const int32_t* __restrict__ trip_ptr,
                                                       const int32_t* __restrict__ trip_l, const int32_t* __restrict__ trip_u,
                                                       const int32_t* __restrict__ trip_t, const S* __restrict__ A, const int16_t* __restrict__ rowlen,
                                                       S* __restrict__ lu, int32_t* __restrict__ flags, const int8_t* __restrict__ simple_row, int copy_upper)
{
    // grid-stride over the level's rows (factor() launches one thread per row; a launch capped to a fraction of the device, for a
    // factorisation on its side stream, changed nothing: DESIGN section 11)
  for (int row = lo + blockIdx.x * kBlock + threadIdx.x; row < hi; row += gridDim.x * kBlock) {
    const int base = slice_ptr[row >> 6], lane = row & 63, nl = nlower[row];
    const int len = rowlen[row];
    const int32_t ed = (base + nl) * 64 + lane;
    int tp = trip_ptr[row];
    const int te = trip_ptr[row + 1];
    // Fast path (every row of a multicolour ordering on a grid stencil): all updates of this row hit its diagonal block, so the
    // diagonal is accumulated in registers and every entry of A is read once and every entry of LU written once -- the generic
    // path below goes through memory for each update (copy, re-load, store; measured 2.6x the traffic of this one).
    const bool simple = simple_row[row] != 0;
    S m[9], o[9];
    if (simple) {
        ld9(A, ed, m);
        for (int k = 0; k < nl; ++k) {
            const int32_t e = (base + k) * 64 + lane;
            const int j = col[e];
            const int32_t ej = (slice_ptr[j >> 6] + nlower[j]) * 64 + (j & 63);
            S a[9], dj[9], L[9];
            ld9(A, e, a); ld9(lu, ej, dj);
            mm9(a, dj, L);
            st9(lu, e, L);
            const S* usrc = simple_row[j] ? A : lu;          // row j's U entries: not copied when they equal A's
            while (tp < te && trip_l[tp] == e) {
                S u[9], bb[9];
                ld9(usrc, trip_u[tp], u);
                mm9(L, u, bb);
#pragma unroll
                for (int q = 0; q < 9; ++q) m[q] -= bb[q];
                ++tp;
            }
        }
        if (copy_upper)
            for (int k = nl + 1; k < len; ++k) {       // upper part: unchanged copy of A -- k_ilu_upper reads it from A, so only on request (get_lu_bsr)
                const int32_t e = (base + k) * 64 + lane;
                S t[9]; ld9(A, e, t); st9(lu, e, t);
            }
    } else {
        // generic IKJ: this row of LU starts as a copy of the row of A, updates go through memory
        for (int k = 0; k < len; ++k) {
            const int32_t e = (base + k) * 64 + lane;
            S t[9]; ld9(A, e, t); st9(lu, e, t);
        }
        for (int k = 0; k < nl; ++k) {
            const int32_t e = (base + k) * 64 + lane;
            const int j = col[e];
            const int32_t ej = (slice_ptr[j >> 6] + nlower[j]) * 64 + (j & 63);
            S a[9], dj[9], L[9];
            ld9(lu, e, a); ld9(lu, ej, dj);
            mm9(a, dj, L);
            st9(lu, e, L);
            const S* usrc = simple_row[j] ? A : lu;
            while (tp < te && trip_l[tp] == e) {
                S u[9], t[9], bb[9];
                ld9(usrc, trip_u[tp], u); ld9(lu, trip_t[tp], t);
                mm9(L, u, bb);
#pragma unroll
                for (int q = 0; q < 9; ++q) t[q] -= bb[q];
                st9(lu, trip_t[tp], t);
                ++tp;
            }
        }
        ld9(lu, ed, m);
    }
    const S c0 = m[4] * m[8] - m[5] * m[7], c1 = m[5] * m[6] - m[3] * m[8], c2 = m[3] * m[7] - m[4] * m[6];
    const S det = m[0] * c0 + m[1] * c1 + m[2] * c2;
    if (det == S(0) || !(det == det)) { atomicOr(flags, 1); continue; }
    const S id = S(1) / det;
    o[0] = c0 * id; o[1] = (m[2] * m[7] - m[1] * m[8]) * id; o[2] = (m[1] * m[5] - m[2] * m[4]) * id;
    o[3] = c1 * id; o[4] = (m[0] * m[8] - m[2] * m[6]) * id; o[5] = (m[2] * m[3] - m[0] * m[5]) * id;
    o[6] = c2 * id; o[7] = (m[1] * m[6] - m[0] * m[7]) * id; o[8] = (m[0] * m[4] - m[1] * m[3]) * id;
    st9(lu, ed, o);
  }
}

template <class S>
__global__ __launch_bounds__(kBlock) void k_dot(long n, const S* __restrict__ a, const S* __restrict__ b, double* __restrict__ partials)
{
    __shared__ double sm[8];
    double acc[1] = { 0.0 };
    constexpr int L = 16 / sizeof(S);              // 16-byte lanes; a fixed summation order
    struct alignas(16) Pack { S v[L]; };
    const long nv = ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) ? 0 : n / L;
    for (long q = blockIdx.x * long(kBlock) + threadIdx.x; q < nv; q += long(gridDim.x) * kBlock) {
        const Pack x4 = reinterpret_cast<const Pack*>(a)[q], y4 = reinterpret_cast<const Pack*>(b)[q];
#pragma unroll
        for (int u = 0; u < L; ++u) acc[0] += double(x4.v[u]) * double(y4.v[u]);
    }
    for (long i = nv * L + blockIdx.x * long(kBlock) + threadIdx.x; i < n; i += long(gridDim.x) * kBlock) acc[0] += double(a[i]) * double(b[i]);
    block_sum<1>(acc, sm);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc[0];
}
// <a, b> over the OWNED rows only (multi-GPU GMRES: the basis vectors carry halo-exchanged ghost entries); mask per row, three planes of nbp
template <class S>
__global__ __launch_bounds__(kBlock) void k_dot_owned(long n, int nbp, const int8_t* __restrict__ mask, const S* __restrict__ a, const S* __restrict__ b,
                                                      double* __restrict__ partials)
{
    __shared__ double sm[8];
    double acc[1] = { 0.0 };
    for (long i = blockIdx.x * long(kBlock) + threadIdx.x; i < n; i += long(gridDim.x) * kBlock) if (mask[i % nbp]) acc[0] += double(a[i]) * double(b[i]);
    block_sum<1>(acc, sm);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc[0];
}
template <class S>
__global__ __launch_bounds__(kBlock) void k_axpy(long n, S a, const S* __restrict__ x, S* __restrict__ y)
{
    for (long i = blockIdx.x * long(kBlock) + threadIdx.x; i < n; i += long(gridDim.x) * kBlock) y[i] += a * x[i];
}
template <class A, class B>
__global__ __launch_bounds__(kBlock) void k_convert(long n, const A* __restrict__ a, B* __restrict__ b)
{
    for (long i = blockIdx.x * long(kBlock) + threadIdx.x; i < n; i += long(gridDim.x) * kBlock) b[i] = B(a[i]);
}
__global__ __launch_bounds__(kBlock) void k_copy16(long n16, const double2* __restrict__ a, double2* __restrict__ b)
{
    for (long i = blockIdx.x * long(kBlock) + threadIdx.x; i < n16; i += long(gridDim.x) * kBlock) b[i] = a[i];
}

// ---- layout conversion kernels ----
__global__ __launch_bounds__(kBlock) void k_bsr_to_sell(int nentries, const int32_t* __restrict__ src, const double* __restrict__ bsr, double* __restrict__ sell)
{
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= nentries) return;
    const int s = src[e];
    double* o = sell + long(e >> 6) * 576 + (e & 63);
#pragma unroll
    for (int q = 0; q < 9; ++q) o[q * 64] = s >= 0 ? bsr[long(s) * 9 + q] : 0.0;
}
template <class S>
__global__ __launch_bounds__(kBlock) void k_sell_to_bsr(int nnzb, const int32_t* __restrict__ entry_of_block, const S* __restrict__ sell, double* __restrict__ bsr)
{
    const int b = blockIdx.x * kBlock + threadIdx.x;
    if (b >= nnzb) return;
    const int e = entry_of_block[b];
    const S* o = sell + long(e >> 6) * 576 + (e & 63);
#pragma unroll
    for (int q = 0; q < 9; ++q) bsr[long(b) * 9 + q] = double(o[q * 64]);
}
template <class S>
__global__ __launch_bounds__(kBlock) void k_vec_in(int nb, int nbp, int layout, const int32_t* __restrict__ nat, const double* __restrict__ h, S* __restrict__ d)
{
    const int r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= nb) return;
    const int c = nat[r];
#pragma unroll
    for (int k = 0; k < 3; ++k) d[long(k) * nbp + r] = S(layout == VEC_BLOCK_INTERLEAVED ? h[3 * long(c) + k] : h[long(k) * nb + c]);
}
template <class S>
__global__ __launch_bounds__(kBlock) void k_vec_out(int nb, int nbp, int layout, const int32_t* __restrict__ nat, const S* __restrict__ d, double* __restrict__ h)
{
    const int r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= nb) return;
    const int c = nat[r];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double val = double(d[long(k) * nbp + r]);
        if (layout == VEC_BLOCK_INTERLEAVED) h[3 * long(c) + k] = val; else h[long(k) * nb + c] = val;
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
void DevPlan::upload(const Plan& P, hipStream_t s)
{
    nb = P.nb; nbp = P.nbp; nslices = P.nslices; nentries = P.nentries; nlevels = P.nlevels; nnzb = P.nnzb;
    slice_ptr.upload(P.slice_ptr, s); col.upload(P.sell_col, s); src.upload(P.sell_src, s);
    entry_of_block.upload(P.entry_of_block, s); nat.upload(P.nat, s); pos.upload(P.pos, s);
    trip_ptr.upload(P.trip_ptr, s);
    std::vector<int32_t> one(1, 0);      // hipMalloc(0) is avoided: keep at least one element
    trip_l.upload(P.trip_l.empty() ? one : P.trip_l, s); trip_u.upload(P.trip_u.empty() ? one : P.trip_u, s);
    trip_t.upload(P.trip_t.empty() ? one : P.trip_t, s);
    rowlen.upload(P.rowlen, s); nlower.upload(P.nlower, s); tpos.upload(P.tpos, s); simple.upload(P.simple, s);
    flux_perm.upload(P.flux_perm, s);
    level_ptr = P.level_ptr;
    OPMGPU_HIP(hipStreamSynchronize(s));      // the host vectors may go away
}

LinSolver::LinSolver(hipStream_t s) : stream(s)
{
    kt.stream = s;
    npart = kMaxPart + kBndPart;
    partials.alloc(size_t(6) * npart + 16 + 3 * 64);       // + three coarse-space vectors riding on the scalar all-reduces (cs_recur)
    flags.alloc(4);
    partials.zero(stream); flags.zero(stream);
    OPMGPU_HIP(hipHostMalloc(reinterpret_cast<void**>(&h_ctl), sizeof(SolveCtl), hipHostMallocMapped));
    std::memset(h_ctl, 0, sizeof(SolveCtl));
    OPMGPU_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&h_ctl_dev), h_ctl, 0));
    OPMGPU_HIP(hipHostMalloc(reinterpret_cast<void**>(&h_tick), sizeof(int), hipHostMallocMapped));
    *h_tick = 0;
    OPMGPU_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&h_tick_dev), h_tick, 0));
    OPMGPU_HIP(hipHostMalloc(reinterpret_cast<void**>(&h_pub), kPubWords * sizeof(uint32_t), hipHostMallocMapped));
    OPMGPU_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&h_pub_dev), h_pub, 0));
    poll_status = env_flag("OPMGPU_POLL", poll_status);
    ctl.alloc(1); ctl.zero(stream);
    OPMGPU_HIP(hipHostMalloc(reinterpret_cast<void**>(&h_flags), 4 * sizeof(int32_t)));
    OPMGPU_HIP(hipEventCreateWithFlags(&ev[0], hipEventDisableTiming));
    OPMGPU_HIP(hipEventCreateWithFlags(&ev[1], hipEventDisableTiming));
    closed_form_level0 = env_flag("OPMGPU_CLOSED", closed_form_level0);
    lean_solve = env_flag("OPMGPU_LEAN_SOLVE", lean_solve);
    cpr_cancel_p = env_flag("OPMGPU_CPR_CANCEL_P", cpr_cancel_p);
    cpr_factor_p = env_flag("OPMGPU_CPR_FACTOR_P", cpr_factor_p);
    well_woodbury = env_flag("OPMGPU_WELL_WOODBURY", well_woodbury);
    cpr_speculate = env_flag("OPMGPU_CPR_SPECULATE", cpr_speculate);
    cpr_weight_mode = env_int("OPMGPU_CPR_WEIGHTS", cpr_weight_mode);
    amg_lag = env_int("OPMGPU_AMG_LAG", amg_lag);
    coarse_lag = std::max(0, env_int("OPMGPU_AMG_LAG_COARSE", coarse_lag));
    cs_blocks_req = std::max(1, env_int("OPMGPU_COARSE_BLOCKS", cs_blocks_req));
    cpr_halo_xp = env_flag("OPMGPU_CPR_HALO_XP", cpr_halo_xp);
    halo_overlap = env_flag("OPMGPU_HALO_OVERLAP", halo_overlap);
    factor_overlap = env_flag("OPMGPU_FACTOR_OVERLAP", factor_overlap);
    factor_early_on = env_flag("OPMGPU_FACTOR_EARLY", factor_early_on);
    cs_recur = env_flag("OPMGPU_CS_RECUR", cs_recur);
    if (const char* e = std::getenv("OPMGPU_CPR_L0_HALO")) { cpr_l0_halo = std::atoi(e) != 0; cpr_l0_halo_down = std::atoi(e) != 2; }
    corr_policy.on = env_flag("OPMGPU_AMG_ADAPT", corr_policy.on);
    if (const char* e = std::getenv("OPMGPU_AMG_ADAPT_ARM")) corr_policy.arm[CorrectionPolicy::kBase + 1] = std::atof(e);
    if (const char* e = std::getenv("OPMGPU_AMG_ADAPT_MARGIN")) corr_policy.margin = std::atof(e);
    emulate_ranks = env_int("OPMGPU_EMULATE_RANKS", emulate_ranks);
    emulate_what = env_int("OPMGPU_EMULATE_WHAT", emulate_what);
    coarse_mode = env_int("OPMGPU_COARSE", coarse_mode);
}
bool LinSolver::plain_setup() const
{
    return !comm && emulate_ranks <= 1 && fill_level == 0 && !now.point_stage2 && !(well_woodbury && wb_active);
}
LinSolver::~LinSolver()
{
    if (h_ctl) (void)hipHostFree(h_ctl);
    if (h_tick) (void)hipHostFree(h_tick);
    if (h_pub) (void)hipHostFree(h_pub);
    if (h_flags) (void)hipHostFree(h_flags);
    if (ev[0]) (void)hipEventDestroy(ev[0]);
    if (ev[1]) (void)hipEventDestroy(ev[1]);
    for (auto e : ev_halo) if (e) (void)hipEventDestroy(e);
    if (halo_stream) (void)hipStreamDestroy(halo_stream);
    for (auto e : ev_factor) if (e) (void)hipEventDestroy(e);
    if (factor_stream) (void)hipStreamDestroy(factor_stream);
}

template <> SolverWork<double>& LinSolver::work<double>() { return wd; }
template <> SolverWork<float>& LinSolver::work<float>() { return wf; }

int LinSolver::set_pattern(int nb, const int32_t* rowptr, const int32_t* col, int ordering)
{
    if (plan.nb == nb && cur_ordering == ordering && plan.nnzb == rowptr[nb] &&
        std::memcmp(plan.rowptr.data(), rowptr, sizeof(int32_t) * (nb + 1)) == 0 &&
        std::memcmp(plan.col.data(), col, sizeof(int32_t) * plan.nnzb) == 0)
        return OPMGPU_OK;
    light_ok_for = nullptr; cs_for = nullptr;        // row numbering changes: the masks / subdomain maps built for the old plan are stale
    Plan P;
    const int st = build_plan(nb, rowptr, col, ordering, P);
    if (st != OPMGPU_OK) return st;
    plan.rowptr.clear();
    plan = std::move(P);
    cur_ordering = ordering;
    ++plan_id;
    dp.upload(plan, stream);
    Ad.alloc(size_t(plan.nentries) * 9);
    Ad.zero(stream);
    wd.allocated = false; wf.allocated = false;
    return OPMGPU_OK;
}

template <class S> void LinSolver::ensure_work()
{
    SolverWork<S>& w = work<S>();
    if (w.allocated) return;
    const size_t nv = size_t(3) * plan.nbp, nm = size_t(plan.nentries) * 9;
    if (sizeof(S) == 4) { w.A.alloc(nm); w.A.zero(stream); }
    w.LU.alloc(nm); w.LU.zero(stream);
    DevArray<S>* vs[] = { &w.r, &w.rt, &w.p, &w.v, &w.t, &w.y, &w.x, &w.b, &w.z, &w.hx };
    for (DevArray<S>* a : vs) { a->alloc(nv); a->zero(stream); }
    w.amg.reset();
    w.allocated = true;
}

void LinSolver::load_host_bsr(const double* val9)
{
    matrix_is_float = false; weights_from_assembly = false; float_copy_valid = false;
    new_step_hint = true;          // an external matrix: nothing is known about its relation to the previous one
    // every external matrix is its own "time step" with a single solve, which the correction-factor policy never scores -- one failed
    // solve would park it on the unscored larger factor for good: external matrices run the fixed first setting
    corr_policy.external = true; corr_policy.cur = CorrectionPolicy::kBase;
    stage.ensure(std::max(size_t(plan.nnzb) * 9, size_t(3) * plan.nbp));
    OPMGPU_HIP(hipMemcpyAsync(stage.p, val9, size_t(plan.nnzb) * 9 * sizeof(double), hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_bsr_to_sell, dim3(grid_for(plan.nentries)), dim3(kBlock), 0, stream, plan.nentries, dp.src.p, stage.p, Ad.p);
}

float* LinSolver::matrix_f() { ensure_work<float>(); return wf.A.p; }
void LinSolver::widen_matrix()
{
    if (!matrix_is_float) return;
    const long n = long(plan.nentries) * 9;
    hipLaunchKernelGGL((k_convert<float, double>), dim3(std::min(grid_for(n), kMaxRedBlocks)), dim3(kBlock), 0, stream, n, (const float*)wf.A.p, Ad.p);
    matrix_is_float = false;
}
template <> void LinSolver::prepare<double>(bool matrix_changed) { ensure_work<double>(); widen_matrix(); if (matrix_changed) pre_stale = true; }
template <> void LinSolver::prepare<float>(bool matrix_changed)
{
    ensure_work<float>();
    if (matrix_changed) pre_stale = true;
    if (!matrix_changed || matrix_is_float) return;
    const long n = long(plan.nentries) * 9;
    hipLaunchKernelGGL((k_convert<double, float>), dim3(std::min(grid_for(n), kMaxRedBlocks)), dim3(kBlock), 0, stream, n, Ad.p, wf.A.p);
}
template <> const double* LinSolver::matrix<double>() { return Ad.p; }
template <> const float* LinSolver::matrix<float>() { return wf.A.p; }

// Diagnostic (OPMGPU_EMULATE_RANKS=N, single GPU): the preconditioner is built from a copy of the matrix whose blocks across the
// cuts of an N-slab decomposition (contiguous caller-index ranges, like slab_partition) are zeroed -- block-Jacobi ILU0 and a
// subdomain-local AMG, i.e. the iteration counts of an N-rank run without N GPUs.  The operator itself stays the full matrix.
template <class S>
__global__ __launch_bounds__(kBlock) void k_cut_copy(int nb, int nranks, const int32_t* __restrict__ slice_ptr, const int32_t* __restrict__ col,
                                                     const int32_t* __restrict__ nat, const S* __restrict__ A, S* __restrict__ out)
{
    const int row = blockIdx.x * kBlock + threadIdx.x;
    if (row >= nb) return;
    const int base = slice_ptr[row >> 6], width = slice_ptr[(row >> 6) + 1] - base, lane = row & 63;
    const long mine = long(nat[row]) * nranks / nb;
    for (int k = 0; k < width; ++k) {
        const long e = long(base + k) * 64 + lane;
        const bool keep = long(nat[col[e]]) * nranks / nb == mine;
        const S* b = A + (e >> 6) * 576 + (e & 63);
        S* o = out + (e >> 6) * 576 + (e & 63);
#pragma unroll
        for (int q = 0; q < 9; ++q) o[q * 64] = keep ? b[q * 64] : S(0);
    }
}
template <class S> const S* LinSolver::pre_matrix()
{
    if (emulate_ranks <= 1) return matrix<S>();
    SolverWork<S>& w = work<S>();
    w.Apre.alloc(size_t(plan.nentries) * 9);
    if (pre_stale) {
        hipLaunchKernelGGL((k_cut_copy<S>), dim3(grid_for(plan.nb)), dim3(kBlock), 0, stream, plan.nb, emulate_ranks, dp.slice_ptr.p, dp.col.p, dp.nat.p,
                           matrix<S>(), w.Apre.p);
        pre_stale = false;
    }
    return w.Apre.p;
}

// ---- the wells in stage 2: local Woodbury correction of the ILU0 application (linsolver.hpp) ----
template <class S>
__global__ __launch_bounds__(kBlock) void k_wb_setup(LowRankOp lr, const int32_t* __restrict__ slice_ptr, const int16_t* __restrict__ nlower,
                                                     const S* __restrict__ lu, double relax, double* __restrict__ Y, double* __restrict__ Ginv)
{
    __shared__ double sm[28];
    __shared__ double G[49];
    const int w = blockIdx.x, tid = threadIdx.x;
    double acc[49];
#pragma unroll
    for (int q = 0; q < 49; ++q) acc[q] = 0.0;
    for (int j = lr.connpos[w] + tid; j < lr.connpos[w + 1]; j += kBlock) {
        const int row = lr.perf_row[j];
        const S* __restrict__ d = lu + vidx(slice_ptr[row >> 6] + nlower[row], row & 63);       // the ILU0's inverted diagonal block, row-major planes
        double Di[9];
#pragma unroll
        for (int q = 0; q < 9; ++q) Di[q] = double(d[q * 64]);
        const double* __restrict__ P = lr.P + 21 * long(j);
        const double* __restrict__ Q = lr.Q + 21 * long(j);
        double y[21];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int k = 0; k < 7; ++k) y[7 * a + k] = relax * (Di[3 * a] * P[k] + Di[3 * a + 1] * P[7 + k] + Di[3 * a + 2] * P[14 + k]);
#pragma unroll
        for (int q = 0; q < 21; ++q) Y[21 * long(j) + q] = y[q];
#pragma unroll
        for (int k = 0; k < 7; ++k)
#pragma unroll
            for (int l = 0; l < 7; ++l) acc[7 * k + l] += Q[3 * k] * y[l] + Q[3 * k + 1] * y[7 + l] + Q[3 * k + 2] * y[14 + l];
    }
    for (int k = 0; k < 7; ++k) {
        double part[7];
#pragma unroll
        for (int l = 0; l < 7; ++l) part[l] = acc[7 * k + l];
        __syncthreads();
        block_sum<7>(part, sm);
        if (tid == 0) for (int l = 0; l < 7; ++l) G[7 * k + l] = part[l] + (k == l ? 1.0 : 0.0);
    }
    __syncthreads();
    if (tid == 0) {
        // Gauss-Jordan with partial pivoting on [G | I]; a singular G switches the correction of this well off (zero inverse)
        double M[7][14];
        for (int r = 0; r < 7; ++r) for (int c = 0; c < 7; ++c) { M[r][c] = G[7 * r + c]; M[r][7 + c] = r == c ? 1.0 : 0.0; }
        bool ok = true;
        for (int c = 0; c < 7 && ok; ++c) {
            int pr = c; double best = fabs(M[c][c]);
            for (int r = c + 1; r < 7; ++r) if (fabs(M[r][c]) > best) { best = fabs(M[r][c]); pr = r; }
            if (!(best > 1e-300)) { ok = false; break; }
            if (pr != c) for (int q = 0; q < 14; ++q) { const double tmp = M[c][q]; M[c][q] = M[pr][q]; M[pr][q] = tmp; }
            const double ip = 1.0 / M[c][c];
            for (int q = 0; q < 14; ++q) M[c][q] *= ip;
            for (int r = 0; r < 7; ++r) if (r != c) { const double f = M[r][c]; if (f != 0.0) for (int q = 0; q < 14; ++q) M[r][q] -= f * M[c][q]; }
        }
        for (int r = 0; r < 7; ++r) for (int c = 0; c < 7; ++c) { const double v = ok ? M[r][7 + c] : 0.0; Ginv[49 * long(w) + 7 * r + c] = (v == v) ? v : 0.0; }
    }
}
template <class S>
__global__ __launch_bounds__(kBlock) void k_wb_apply(LowRankOp lr, int nbp, const double* __restrict__ Y, const double* __restrict__ Ginv, S* __restrict__ v,
                                                     const SolveCtl* __restrict__ ctl)
{
    __shared__ double sm[28];
    __shared__ double ts[7], ss[7];
    if (ctl && ctl->done) return;
    const int w = blockIdx.x, tid = threadIdx.x;
    double acc[7] = { 0, 0, 0, 0, 0, 0, 0 };
    for (int j = lr.connpos[w] + tid; j < lr.connpos[w + 1]; j += kBlock) {
        const int row = lr.perf_row[j];
        const double x0 = double(v[row]), x1 = double(v[nbp + row]), x2 = double(v[2 * long(nbp) + row]);
        const double* __restrict__ Q = lr.Q + 21 * long(j);
#pragma unroll
        for (int k = 0; k < 7; ++k) acc[k] += Q[3 * k] * x0 + Q[3 * k + 1] * x1 + Q[3 * k + 2] * x2;
    }
    block_sum<7>(acc, sm);
    if (tid == 0) for (int k = 0; k < 7; ++k) ts[k] = acc[k];
    __syncthreads();
    if (tid < 7) { double s = 0.0; for (int l = 0; l < 7; ++l) s += Ginv[49 * long(w) + 7 * tid + l] * ts[l]; ss[tid] = s; }
    __syncthreads();
    for (int j = lr.connpos[w] + tid; j < lr.connpos[w + 1]; j += kBlock) {
        const int row = lr.perf_row[j];
        const double* __restrict__ y = Y + 21 * long(j);
        double d0 = 0.0, d1 = 0.0, d2 = 0.0;
#pragma unroll
        for (int k = 0; k < 7; ++k) { d0 += y[k] * ss[k]; d1 += y[7 + k] * ss[k]; d2 += y[14 + k] * ss[k]; }
        v[row] -= S(d0); v[nbp + row] -= S(d1); v[2 * long(nbp) + row] -= S(d2);
    }
}

template <> LinSolver::FillWork<float>& LinSolver::FillIlu::work<float>() { return wf; }
template <> LinSolver::FillWork<double>& LinSolver::FillIlu::work<double>() { return wd; }

template <class S> int LinSolver::factor(bool wait)
{
    if (fill_level > 0) return fill_factor<S>(wait);
    SolverWork<S>& w = work<S>();
    KtScope kts(kt, KT_ILU_FACTOR);
    flags.zero(stream);
    for (int l = 0; l < plan.nlevels; ++l) {
        const int lo = plan.level_ptr[l], hi = plan.level_ptr[l + 1];
        if (hi == lo) continue;
        hipLaunchKernelGGL((k_ilu_factor<S>), dim3(grid_for(hi - lo)), dim3(kBlock), 0, stream, lo, hi, dp.slice_ptr.p, dp.col.p,
                           dp.nlower.p, dp.trip_ptr.p, dp.trip_l.p, dp.trip_u.p, dp.trip_t.p, ((emulate_what & 1) ? pre_matrix<S>() : matrix<S>()), dp.rowlen.p, w.LU.p, flags.p,
                           (const int8_t*)dp.simple.p, int(lu_copy_upper));
    }
    if (well_woodbury && lowrank.nw > 0 && lowrank.P && !comm) {
        // the wells' Woodbury data of this factorisation (same stream: ordered behind it, covered by join_factor like the factors)
        wb_buf.ensure(size_t(21) * lowrank.nperf + size_t(49) * lowrank.nw);
        hipLaunchKernelGGL((k_wb_setup<S>), dim3(lowrank.nw), dim3(kBlock), 0, stream, lowrank, dp.slice_ptr.p, dp.nlower.p, (const S*)w.LU.p, wb_relax,
                           wb_buf.p, wb_buf.p + size_t(21) * lowrank.nperf);
    }
    OPMGPU_HIP(hipMemcpyAsync(h_flags, flags.p, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    if (!wait) return OPMGPU_OK;          // the caller reads factor_status() after its next synchronisation (no pipeline bubble per solve)
    OPMGPU_HIP(hipStreamSynchronize(stream));
    return factor_status();
}

template <class S> void LinSolver::factor_async()
{
    if (!factor_stream) {
        // lowest priority: the factorisation is needed only by the first ILU0 sweep (behind the hierarchy set-up AND the first V-cycle),
        // the Galerkin chain next to it is the critical path -- the dispatcher should give that one the free slots first
        static const bool low = env_flag("OPMGPU_FACTOR_PRIORITY", true);
        int least = 0, greatest = 0;
        OPMGPU_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
        OPMGPU_HIP(hipStreamCreateWithPriority(&factor_stream, hipStreamNonBlocking, low ? least : greatest));
        for (auto& e : ev_factor) OPMGPU_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    OPMGPU_HIP(hipEventRecord(ev_factor[0], stream));
    OPMGPU_HIP(hipStreamWaitEvent(factor_stream, ev_factor[0], 0));
    {
        StreamSwapGuard g(stream, factor_stream, kt.on);  // (event brackets belong to the main stream); restored also if factor() throws
        (void)factor<S>(false);
    }
    OPMGPU_HIP(hipEventRecord(ev_factor[1], factor_stream));
    factor_pending = true;
}
void LinSolver::join_factor()
{
    if (!factor_pending) return;
    OPMGPU_HIP(hipStreamWaitEvent(stream, ev_factor[1], 0));
    factor_pending = false;
}

// d0, xp (CPR with cancel_p_now; cpr_apply has checked the plan and the factors): d = d0 - A [xp; 0; 0] is the second stage's input, d0 the
// application's.  v = [xp; 0; 0] + (LU)^-1 d without a pass of its own for the sum: the top level's rows add xp as they become final, a
// level-0 row r has D_r = A_rr and U_rb = A_rb, so its entry of the SUM is D_r^-1 (d0_r - sum_b A_rb v_b) with v_b the final top-level entries.
// a_fp (cpr_factor_p, with d0 and xp; a two-level plan): the unfactorised matrix.  d then holds, on the level-0 rows only, the residual
// without its diagonal term; the top level's sweep forms its rows' right-hand side from d0, xp and a_fp (k_ilu_lower, FP)
template <class S> void LinSolver::ilu_apply(const S* d, S* v, double relax, const SolveCtl* ctl, const S* d0, const S* xp, const S* a_fp)
{
    join_factor();
    KtScope kts(kt, KT_ILU_APPLY);
    if (fill_level > 0) { fill_apply<S>(d, v, relax, ctl); return; }
    SolverWork<S>& w = work<S>();
    const int L = plan.nlevels;
    const int n0 = plan.level_ptr[1];
    if (L == 1) {
        hipLaunchKernelGGL((k_ilu_lower<S>), dim3(grid8_for(n0)), dim3(kBlock), 0, stream, xcd_mode(), 0, n0, 0, plan.nbp, 1, S(relax),
                           dp.slice_ptr.p, dp.col.p, dp.nlower.p, w.LU.p, d, v, ctl);
        return;
    }
    for (int l = 1; l < L; ++l) {
        const int lo = plan.level_ptr[l], hi = plan.level_ptr[l + 1];
        if (hi == lo) continue;
        if (a_fp && d0 && xp && L == 2)
            hipLaunchKernelGGL((k_ilu_lower<S, true>), dim3(grid8_for(hi - lo)), dim3(kBlock), 0, stream, xcd_mode(), lo, hi, n0, plan.nbp, 1, S(relax),
                               dp.slice_ptr.p, dp.col.p, dp.nlower.p, w.LU.p, d0, v, ctl, xp, a_fp, d);
        else
            hipLaunchKernelGGL((k_ilu_lower<S>), dim3(grid8_for(hi - lo)), dim3(kBlock), 0, stream, xcd_mode(), lo, hi, n0, plan.nbp, int(l == L - 1), S(relax),
                               dp.slice_ptr.p, dp.col.p, dp.nlower.p, w.LU.p, d, v, ctl, xp);
    }
    for (int l = L - 2; l >= 0; --l) {
        const int lo = plan.level_ptr[l], hi = plan.level_ptr[l + 1];
        if (hi == lo) continue;
        hipLaunchKernelGGL((k_ilu_upper<S>), dim3(grid8_for(hi - lo)), dim3(kBlock), 0, stream, xcd_mode(), lo, hi, n0, plan.nbp, S(relax), dp.slice_ptr.p, dp.col.p,
                           dp.nlower.p, dp.rowlen.p, w.LU.p, (l == 0 && d0) ? d0 : d, v, ctl, (const int8_t*)dp.simple.p, ((emulate_what & 1) ? pre_matrix<S>() : matrix<S>()));
    }
}

template <class S> void LinSolver::spmv(const S* x, S* y) { spmv_at<S>(x, y, matrix<S>(), dp.col.p); }

template <class S> void LinSolver::spmv_at(const S* x, S* y, const S* val, const int32_t* col)
{
    const int g = std::min(grid8_for(plan.nb), 4 * kMaxPart);
    lowrank_reduce<S>(x, nullptr);
    hipLaunchKernelGGL((k_spmv<S, 0>), dim3(g), dim3(kBlock), 0, stream, xcd_mode(), plan.nb, plan.nbp, dp.slice_ptr.p, col,
                       val, x, y, (const S*)nullptr, comm ? comm->owner_mask() : (const int8_t*)nullptr, (const SolveCtl*)nullptr,
                       (double*)nullptr, (double*)nullptr, (const S*)nullptr, (const S*)nullptr, 0, S(0), lowrank, (const int8_t*)nullptr);
}

template <class S> void LinSolver::lowrank_reduce(const S* x, const SolveCtl* ctl)
{
    if (lowrank.nw > 0) hipLaunchKernelGGL((k_lowrank_reduce<S>), dim3(lowrank.nw), dim3(kBlock), 0, stream, lowrank, plan.nbp, x, ctl);
}

// the communicator's halo operations by vector type
static void halo(CommBase* c, float* v, hipStream_t s) { c->halo_exchange_f(v, s); }
static void halo(CommBase* c, double* v, hipStream_t s) { c->halo_exchange_d(v, s); }
static void allreduce_halo(CommBase* c, double* d, int n, float* v, hipStream_t s) { c->allreduce_sum_halo_f(d, n, v, s); }
static void allreduce_halo(CommBase* c, double* d, int n, double* v, hipStream_t s) { c->allreduce_sum_halo_d(d, n, v, s); }
// The halo exchange of v on the halo stream next to launch(1), the rows that read no ghost entry; launch(2), the rows next to a cut,
// follows the exchange (LinSolver::halo_overlap)
template <class S, class F> static void halo_overlapped(LinSolver& ls, S* v, F launch)
{
    OPMGPU_HIP(hipEventRecord(ls.ev_halo[0], ls.stream));
    OPMGPU_HIP(hipStreamWaitEvent(ls.halo_stream, ls.ev_halo[0], 0));
    halo(ls.comm, v, ls.halo_stream);
    OPMGPU_HIP(hipEventRecord(ls.ev_halo[1], ls.halo_stream));
    launch(1);
    OPMGPU_HIP(hipStreamWaitEvent(ls.stream, ls.ev_halo[1], 0));
    launch(2);
}

#include "coarse_space.inl"
#include "elliptic.inl"
#include "fillilu.inl"
#include "pointilu.inl"
#include "cpr.inl"

// Wait for the status block of the check kernel just enqueued.  Spinning on a host-mapped word the kernel writes last sees the result
// a few microseconds after the kernel retires; hipStreamSynchronize takes an interrupt round trip (~20 us of idle GPU per check).
// Falls back to the stream synchronisation after 20 ms (a faulted kernel never ticks; the synchronisation then reports the error).
void LinSolver::wait_tick(int tick)
{
    if (poll_status) {
        const auto t0 = std::chrono::steady_clock::now();
        volatile int* t = h_tick;
        for (long spins = 0; *t != tick; ++spins) {
            if ((spins & 1023) == 1023 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) break;
            __builtin_ia32_pause();
        }
        if (*t == tick) { std::atomic_thread_fence(std::memory_order_acquire); return; }
    }
    OPMGPU_HIP(hipStreamSynchronize(stream));
}

__global__ __launch_bounds__(kBlock) void k_fetch_words(const uint32_t* __restrict__ s0, int n0, const uint32_t* __restrict__ s1, int n1, const uint32_t* __restrict__ s2, int n2,
                                                        uint32_t* __restrict__ dst, int* __restrict__ tick_ptr, int tick)
{
    for (int i = threadIdx.x; i < n0; i += kBlock) dst[i] = s0[i];
    for (int i = threadIdx.x; i < n1; i += kBlock) dst[n0 + i] = s1[i];
    for (int i = threadIdx.x; i < n2; i += kBlock) dst[n0 + n1 + i] = s2[i];
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) { __threadfence_system(); *(volatile int*)tick_ptr = tick; }
}
const uint32_t* LinSolver::fetch_words(const void* src0, int nwords0, const void* src1, int nwords1, const void* src2, int nwords2)
{
    if (nwords0 + nwords1 + nwords2 > kPubWords) throw HipError(OPMGPU_EINVAL, "fetch_words: too many words");
    if (!poll_status) {
        if (nwords0) OPMGPU_HIP(hipMemcpyAsync(h_pub, src0, size_t(nwords0) * 4, hipMemcpyDeviceToHost, stream));
        if (nwords1) OPMGPU_HIP(hipMemcpyAsync(h_pub + nwords0, src1, size_t(nwords1) * 4, hipMemcpyDeviceToHost, stream));
        if (nwords2) OPMGPU_HIP(hipMemcpyAsync(h_pub + nwords0 + nwords1, src2, size_t(nwords2) * 4, hipMemcpyDeviceToHost, stream));
        OPMGPU_HIP(hipStreamSynchronize(stream));
        return h_pub;
    }
    const int tick = ++tick_seq;
    hipLaunchKernelGGL(k_fetch_words, dim3(1), dim3(kBlock), 0, stream, static_cast<const uint32_t*>(src0), nwords0, static_cast<const uint32_t*>(src1), nwords1,
                       static_cast<const uint32_t*>(src2), nwords2, h_pub_dev, h_tick_dev, tick);
    wait_tick(tick);
    return h_pub;
}

// ---- mixed precision: float preconditioner inside a double Krylov method (opmgpu_params.preconditioner_single) ----
void LinSolver::mixed_prepare(bool matrix_changed)
{
    ensure_work<float>();
    if (matrix_is_float) { float_copy_valid = true; return; }        // (a float assembly widened for a double solve: the float buffer is the original)
    if (float_copy_valid && !matrix_changed) return;
    if (!float_copy_valid) {
        const long n = long(plan.nentries) * 9;
        hipLaunchKernelGGL((k_convert<double, float>), dim3(std::min(grid_for(n), kMaxRedBlocks)), dim3(kBlock), 0, stream, n, (const double*)Ad.p, wf.A.p);
        float_copy_valid = true;
    }
}
void LinSolver::cpr_prepare_mixed()
{
    const long n3 = long(3) * plan.nbp;
    const int g = std::min(grid_for(n3), kMaxRedBlocks);
    ensure_work<float>();
    wf.cprw.alloc(size_t(n3));
    if (weights_from_assembly)      // the assembly wrote the 0 / 1 weights next to the double matrix
        hipLaunchKernelGGL((k_convert<double, float>), dim3(g), dim3(kBlock), 0, stream, n3, (const double*)wd.cprw.p, wf.cprw.p);
    cpr_prepare<float>();
    if (!weights_from_assembly) {   // users on the double side (the coarse-space recurrences of a decomposed BiCGStab) read wd.cprw
        wd.cprw.alloc(size_t(n3));
        hipLaunchKernelGGL((k_convert<float, double>), dim3(g), dim3(kBlock), 0, stream, n3, (const float*)wf.cprw.p, wd.cprw.p);
    }
}
template <class S> void LinSolver::precond_apply(const S* d, S* out, double relax, const SolveCtl* ctl, bool cpr, const double* cr_given)
{
    if (!now.mixed || sizeof(S) == 4) {
        if (cpr) cpr_apply<S>(d, out, relax, ctl, cr_given); else ilu_apply<S>(d, out, relax, ctl);
        return;
    }
    const long n = long(3) * plan.nbp;
    const int g = std::min(grid_for(n), kMaxRedBlocks);
    hipLaunchKernelGGL((k_convert<S, float>), dim3(g), dim3(kBlock), 0, stream, n, d, wf.p.p);
    if (cpr) cpr_apply<float>(wf.p.p, wf.y.p, relax, ctl, cr_given); else ilu_apply<float>(wf.p.p, wf.y.p, relax, ctl);
    hipLaunchKernelGGL((k_convert<float, S>), dim3(g), dim3(kBlock), 0, stream, n, (const float*)wf.y.p, out);
}

#include "krylov.inl"
#include "solve.inl"
#include "cpr_inspect.inl"

template <class S> void LinSolver::vec_in(const double* dsrc, int layout, S* d)
{
    hipLaunchKernelGGL((k_vec_in<S>), dim3(grid_for(plan.nb)), dim3(kBlock), 0, stream, plan.nb, plan.nbp, layout, dp.nat.p, dsrc, d);
}
template <class S> void LinSolver::vec_out(const S* d, int layout, double* ddst)
{
    hipLaunchKernelGGL((k_vec_out<S>), dim3(grid_for(plan.nb)), dim3(kBlock), 0, stream, plan.nb, plan.nbp, layout, dp.nat.p, d, ddst);
}
template <class S> void LinSolver::vec_from_host(const double* h, int layout, S* d)
{
    stage.ensure(std::max(size_t(plan.nnzb) * 9, size_t(3) * plan.nbp));
    OPMGPU_HIP(hipMemcpyAsync(stage.p, h, size_t(3) * plan.nb * sizeof(double), hipMemcpyHostToDevice, stream));
    vec_in<S>(stage.p, layout, d);
}
template <class S> void LinSolver::vec_to_host(const S* d, int layout, double* h)
{
    stage.ensure(std::max(size_t(plan.nnzb) * 9, size_t(3) * plan.nbp));
    vec_out<S>(d, layout, stage.p);
    OPMGPU_HIP(hipMemcpyAsync(h, stage.p, size_t(3) * plan.nb * sizeof(double), hipMemcpyDeviceToHost, stream));
    OPMGPU_HIP(hipStreamSynchronize(stream));
}

void LinSolver::get_matrix_bsr(const double* sell, double* val9)
{
    stage.ensure(std::max(size_t(plan.nnzb) * 9, size_t(3) * plan.nbp));
    hipLaunchKernelGGL((k_sell_to_bsr<double>), dim3(grid_for(plan.nnzb)), dim3(kBlock), 0, stream, plan.nnzb, dp.entry_of_block.p, sell, stage.p);
    OPMGPU_HIP(hipMemcpyAsync(val9, stage.p, size_t(plan.nnzb) * 9 * sizeof(double), hipMemcpyDeviceToHost, stream));
    OPMGPU_HIP(hipStreamSynchronize(stream));
}
// mixed precision: the float copy of the double matrix as it stands (valid or not: the caller checks float_copy_valid), widened
void LinSolver::get_float_copy_bsr(double* val9)
{
    stage.ensure(std::max(size_t(plan.nnzb) * 9, size_t(3) * plan.nbp));
    hipLaunchKernelGGL((k_sell_to_bsr<float>), dim3(grid_for(plan.nnzb)), dim3(kBlock), 0, stream, plan.nnzb, dp.entry_of_block.p, (const float*)matrix_f(), stage.p);
    OPMGPU_HIP(hipMemcpyAsync(val9, stage.p, size_t(plan.nnzb) * 9 * sizeof(double), hipMemcpyDeviceToHost, stream));
    OPMGPU_HIP(hipStreamSynchronize(stream));
}
template <class S> void LinSolver::get_lu_bsr(double* val9)
{
    // the solver's factorisation leaves out the U entries that equal A's (k_ilu_upper reads those from A): factorise once more in full
    lu_copy_upper = true;
    (void)factor<S>(true);
    lu_copy_upper = false;
    stage.ensure(std::max(size_t(plan.nnzb) * 9, size_t(3) * plan.nbp));
    hipLaunchKernelGGL((k_sell_to_bsr<S>), dim3(grid_for(plan.nnzb)), dim3(kBlock), 0, stream, plan.nnzb, dp.entry_of_block.p, work<S>().LU.p, stage.p);
    OPMGPU_HIP(hipMemcpyAsync(val9, stage.p, size_t(plan.nnzb) * 9 * sizeof(double), hipMemcpyDeviceToHost, stream));
    OPMGPU_HIP(hipStreamSynchronize(stream));
}

template <class S> static double time_kernel_t(LinSolver& ls, int kernel, int reps, double relax)
{
    SolverWork<S>& w = ls.work<S>();
    if ((kernel == OPMGPU_K_CPR_APPLY || kernel == OPMGPU_K_VCYCLE) && (!w.amg || !w.amg->ready())) throw HipError(OPMGPU_EINVAL, "no CPR hierarchy yet (solve once with use_cpr)");
    const Plan& P = ls.plan;
    const long n = long(3) * P.nbp;
    const int gv = std::min(grid_for(n), kMaxPart);
    hipEvent_t e0, e1;
    OPMGPU_HIP(hipEventCreate(&e0)); OPMGPU_HIP(hipEventCreate(&e1));
    // OPMGPU_K_SPMV_COLD: kColdCopies copies of (values, column indices), one per launch in turn: together > 4 x the 256 MiB Infinity
    // Cache at 100^3, so every launch streams its matrix from HBM like a solve on a large deck does
    constexpr int kColdCopies = 4;
    const size_t vbytes = size_t(P.nentries) * 9 * sizeof(S), cbytes = (size_t(P.nentries) * sizeof(int32_t) + 255) / 256 * 256;
    if (kernel == OPMGPU_K_SPMV_COLD) {
        ls.cold.alloc(kColdCopies * (vbytes + cbytes));
        for (int c = 0; c < kColdCopies; ++c) {
            OPMGPU_HIP(hipMemcpyAsync(ls.cold.p + c * (vbytes + cbytes), ls.matrix<S>(), vbytes, hipMemcpyDeviceToDevice, ls.stream));
            OPMGPU_HIP(hipMemcpyAsync(ls.cold.p + c * (vbytes + cbytes) + vbytes, ls.dp.col.p, size_t(P.nentries) * sizeof(int32_t), hipMemcpyDeviceToDevice, ls.stream));
        }
    }
    int rot = 0;
    auto launch = [&]() {
        switch (kernel) {
        case OPMGPU_K_SPMV: ls.spmv<S>(w.p.p, w.v.p); break;
        case OPMGPU_K_SPMV_COLD: {
            const char* base = ls.cold.p + (rot++ % kColdCopies) * (vbytes + cbytes);
            ls.spmv_at<S>(w.p.p, w.v.p, reinterpret_cast<const S*>(base), reinterpret_cast<const int32_t*>(base + vbytes));
            break;
        }
        case OPMGPU_K_ILU_APPLY: ls.ilu_apply<S>(w.p.p, w.y.p, relax, nullptr); break;
        case OPMGPU_K_CPR_APPLY: ls.cpr_apply<S>(w.p.p, w.y.p, relax, nullptr); break;
        case OPMGPU_K_VCYCLE: w.amg->vcycle(nullptr, false); break;
        case OPMGPU_K_CPR_SETUP: ls.cpr_prepare<S>(); break;
        case OPMGPU_K_DOT: hipLaunchKernelGGL((k_dot<S>), dim3(gv), dim3(kBlock), 0, ls.stream, n, w.p.p, w.v.p, ls.partials.p); break;
        case OPMGPU_K_AXPY: hipLaunchKernelGGL((k_axpy<S>), dim3(gv), dim3(kBlock), 0, ls.stream, n, S(1e-3), w.p.p, w.t.p); break;
        case OPMGPU_K_STREAM_COPY: {
            const long n16 = long(P.nentries) * 9 * sizeof(S) / 16;
            hipLaunchKernelGGL(k_copy16, dim3(kMaxRedBlocks), dim3(kBlock), 0, ls.stream, n16, reinterpret_cast<const double2*>(ls.matrix<S>()),
                               reinterpret_cast<double2*>(w.LU.p));
            break;
        }
        default: break;
        }
    };
    launch();                                   // warm-up
    OPMGPU_HIP(hipEventRecord(e0, ls.stream));
    for (int i = 0; i < reps; ++i) launch();
    OPMGPU_HIP(hipEventRecord(e1, ls.stream));
    OPMGPU_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    OPMGPU_HIP(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (kernel == OPMGPU_K_SPMV_COLD) ls.cold.release();
    return double(ms) / reps;
}

double LinSolver::time_kernel(int kernel, int reps, int single_precision)
{
    if (kernel == OPMGPU_K_ILU_FACTOR) {
        hipEvent_t e0, e1;
        OPMGPU_HIP(hipEventCreate(&e0)); OPMGPU_HIP(hipEventCreate(&e1));
        if (single_precision) factor<float>(); else factor<double>();
        OPMGPU_HIP(hipEventRecord(e0, stream));
        for (int i = 0; i < reps; ++i) { if (single_precision) factor<float>(); else factor<double>(); }
        OPMGPU_HIP(hipEventRecord(e1, stream));
        OPMGPU_HIP(hipEventSynchronize(e1));
        float ms = 0.f;
        OPMGPU_HIP(hipEventElapsedTime(&ms, e0, e1));
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        return double(ms) / reps;
    }
    return single_precision ? time_kernel_t<float>(*this, kernel, reps, 0.9) : time_kernel_t<double>(*this, kernel, reps, 0.9);
}

// explicit instantiations: what other translation units call; bicgstab and gmres (solve() calls them) stay named symbols of the library
#define OPMGPU_INST(S)                                                                  \
    template void LinSolver::ensure_work<S>();                                           \
    template int LinSolver::factor<S>(bool);                                                 \
    template void LinSolver::ilu_apply<S>(const S*, S*, double, const SolveCtl*, const S*, const S*, const S*);        \
    template void LinSolver::spmv<S>(const S*, S*);                                      \
    template void LinSolver::cpr_reweigh_rows<S>(const int32_t*, int);                   \
    template SolveResult LinSolver::bicgstab<S>(const opmgpu_params&);                   \
    template SolveResult LinSolver::gmres<S>(const opmgpu_params&);                      \
    template int LinSolver::solve<S>(const opmgpu_params&, bool, SolveResult&, std::string&);      \
    template AmgHierarchy<S>* LinSolver::cpr_hierarchy<S>();                             \
    template int LinSolver::cpr_levels<S>(int32_t*, int32_t*, int64_t*, int32_t*);       \
    template int LinSolver::cpr_level_get<S>(int, int32_t*, int32_t*, double*, int32_t*, double*);        \
    template int LinSolver::cpr_dist_level_get<S>(int, int64_t*, int64_t*, int32_t*, int64_t*, double*, int64_t*);        \
    template int LinSolver::cpr_vcycle_apply_host<S>(const double*, double*);            \
    template int LinSolver::cpr_apply_host<S>(const double*, double*, double);           \
    template int LinSolver::cpr_elliptic_ilu_apply_host<S>(const double*, double*);      \
    template void LinSolver::vec_from_host<S>(const double*, int, S*);                   \
    template void LinSolver::vec_to_host<S>(const S*, int, double*);                     \
    template void LinSolver::get_lu_bsr<S>(double*);
OPMGPU_INST(float)
OPMGPU_INST(double)

} // namespace opmgpu
