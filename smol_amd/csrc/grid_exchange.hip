// Replica exchange across a mu-T grid (smolmc_exchange_grid, engine.hip): decided and applied on the device.  A
// translation unit of its own, like walker_mu.hip: a kernel added to engine.hip would move the descriptors of all of
// its kernels.
//
// State point s = (beta_s, row_s).  Walker a at s, walker b at t, H_s(x) = E0(x) - n(x) . row_s, d = row_t - row_s:
//   Delta = (beta_s - beta_t) (Hb - Ha) + beta_s (n_b . d) - beta_t (n_a . d),   accept iff -Delta >= 0 or log u < -Delta
// On acceptance the walkers swap their state points (beta and the row cells the kernels read), the chemical work of a
// gains n_a . d and its enthalpy loses it, b the other way round with n_b . d; occupancies do not move.
// parallel.GridExchange.decide is the same arithmetic in NumPy, operation by operation: the same decisions bit for bit.
// For that every product and every sum of the kernel below must round on its own.  hipcc contracts a * b + c into an
// fma by default, and this toolchain's __dmul_rn / __dadd_rn are plain operators that contract like any other: the
// pragma at the top of the kernel is what keeps them apart (its ISA holds no f64 fma / fmac; check after a change).
#include "smolmc_common.h"

#define GX_WAVES 4 // pairs (waves) per workgroup

struct GridExchangeArgs {
    const uint8_t *occ;
    double *rows;                  // [R][stride]: cell sub * 8 + code, the rows in use; null: one row for all walkers
    double *beta, *enthalpy;       // [R]
    double *features;              // the chemical work is features[r * F + F - 1]
    int32_t *point_of, *walker_at; // walker -> state point, state point -> walker
    const int32_t *pairs;          // [npairs][2] state points
    const double *log_u;           // [npairs]
    int32_t *accepted;             // [npairs] out
    int npairs, Npad, F, stride, nsub;
    int sbase[4], nact[4];
};

// Sum over the 64 lanes, in every lane, without the LDS crossbar: DPP inside a row of 16 (the two quad permutations,
// row_half_mirror, row_mirror: each a full permutation, so no lane reads an invalid one), then the four row sums
// through readlane.  All 64 lanes must be active.
__device__ __forceinline__ int gx_wave_sum(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true);  // quad_perm:[1,0,3,2]
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, true);  // quad_perm:[2,3,0,1]
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, true); // row_half_mirror
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, true); // row_mirror
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) +
           __builtin_amdgcn_readlane(v, 48);
}

// Species counts of row[base .. base + n) over the wave: 16-byte loads of the aligned chunks that cover the range (a
// walker's occupancy row is Npad bytes, Npad a multiple of 16, so every chunk lies inside the row; the bytes of a chunk
// outside the range are not counted).  A lane keeps its counts in eight 8-bit fields of one register and empties them
// into cnt[] every 15 chunks (240 bytes < 256); then one DPP reduction per code.
__device__ __forceinline__ void gx_count(const uint8_t *row, const int base, const int n, const int lane, int (&cnt)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) cnt[j] = 0;
    const int c1 = (base + n + 15) >> 4;
    uint64_t acc = 0;
    int pending = 0;
    for (int c = (base >> 4) + lane; c < c1; c += 64) {
        const uint4 v = *reinterpret_cast<const uint4 *>(row + (size_t)c * 16);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        const int first = c * 16;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int pos = first + i;
            const uint32_t code = (w[i >> 2] >> (8 * (i & 3))) & 7u;
            acc += (uint64_t)(pos >= base && pos < base + n) << (8 * code);
        }
        if (++pending == 15) {
#pragma unroll
            for (int j = 0; j < 8; ++j) cnt[j] += (int)((acc >> (8 * j)) & 255u);
            acc = 0;
            pending = 0;
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) cnt[j] = gx_wave_sum(cnt[j] + (int)((acc >> (8 * j)) & 255u));
}

// one wave per pair; the pairs of a call are disjoint, so no two waves touch the same walker or state point
__global__ void __launch_bounds__(64 * GX_WAVES) grid_exchange_kernel(const GridExchangeArgs A) {
#pragma clang fp contract(off)
    const int p = blockIdx.x * GX_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= A.npairs) return;
    const int s = A.pairs[2 * p], t = A.pairs[2 * p + 1];
    const int a = A.walker_at[s], b = A.walker_at[t];
    const double bs = A.beta[a], bt = A.beta[b], Ha = A.enthalpy[a], Hb = A.enthalpy[b];
    // n_a . d and n_b . d over the cells in ascending order, products and sums rounded one by one
    double wa = 0.0, wb = 0.0;
    if (A.rows) {
        const double *ra = A.rows + (size_t)a * A.stride, *rb = A.rows + (size_t)b * A.stride;
        for (int k = 0; k < A.nsub; ++k) {
            int na[8], nb[8];
            gx_count(A.occ + (size_t)a * A.Npad, A.sbase[k], A.nact[k], lane, na);
            gx_count(A.occ + (size_t)b * A.Npad, A.sbase[k], A.nact[k], lane, nb);
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const double d = rb[k * 8 + c] - ra[k * 8 + c];
                wa = wa + (double)na[c] * d;
                wb = wb + (double)nb[c] * d;
            }
        }
    }
    const double delta = ((bs - bt) * (Hb - Ha) + bs * wb) - bt * wa;
    const bool acc = -delta >= 0.0 || A.log_u[p] < -delta;
    if (acc) {
        if (A.rows && lane < A.stride) { // the two rows change places, a cell per lane
            double *ra = A.rows + (size_t)a * A.stride + lane, *rb = A.rows + (size_t)b * A.stride + lane;
            const double va = *ra, vb = *rb;
            *ra = vb;
            *rb = va;
        }
        if (lane == 0) {
            A.beta[a] = bt;
            A.beta[b] = bs;
            double *fa = A.features + (size_t)a * A.F + A.F - 1, *fb = A.features + (size_t)b * A.F + A.F - 1;
            *fa = *fa + wa;
            *fb = *fb - wb;
            A.enthalpy[a] = Ha - wa;
            A.enthalpy[b] = Hb + wb;
            A.point_of[a] = t;
            A.point_of[b] = s;
            A.walker_at[s] = b;
            A.walker_at[t] = a;
        }
    }
    if (lane == 0) A.accepted[p] = acc ? 1 : 0;
}

int smolmc_grid_exchange_launch(smolmc_handle *h, int npairs, const int32_t *pairs, const double *log_u, int32_t *accepted,
                                int32_t *point_of, int32_t *walker_at) {
    const LeanParams &lp = h->lp;
    GridExchangeArgs A;
    memset(&A, 0, sizeof(A));
    A.occ = h->kp.occ;
    A.rows = lp.mu_stride ? h->d_walker_mu[0] : nullptr;
    A.beta = h->d_beta; A.enthalpy = h->kp.enthalpy; A.features = lp.features;
    A.point_of = point_of; A.walker_at = walker_at; A.pairs = pairs; A.log_u = log_u; A.accepted = accepted;
    A.npairs = npairs; A.Npad = h->Npad; A.F = lp.F; A.stride = lp.mu_stride;
    A.nsub = h->lean_multi() ? lp.m_nsub : 1;
    for (int k = 0; k < A.nsub; ++k) {
        A.sbase[k] = h->lean_multi() ? lp.m_sbase[k] : lp.sbase;
        A.nact[k] = h->lean_multi() ? lp.m_nact[k] : lp.nact;
    }
    hipLaunchKernelGGL(grid_exchange_kernel, dim3((unsigned)((npairs + GX_WAVES - 1) / GX_WAVES)), dim3(64 * GX_WAVES), 0,
                       h->stream, A);
    HIPCHK(hipGetLastError());
    return 0;
}
