// Per-walker chemical potentials (smolmc_set_walker_mu, engine.hip): the re-pricing of the chemical work when the rows
// change.  A translation unit of its own: a kernel added to engine.hip would move the descriptors of all of its kernels.
#include "smolmc_common.h"

struct WalkerMuArgs {
    const uint8_t *occ;
    const double *rows_old, *rows_new; // [R or 1][stride]: cell sub * 8 + code
    double *features, *enthalpy;       // the chemical work is features[r * F + F - 1]; enthalpy may be null
    int R, Npad, F, stride_old, stride_new, nsub;
    int sbase[4], nact[4];
};
// one wave per walker: species counts per sublattice range . (new row - old row) joins the chemical work, and leaves
// the enthalpy with the feature's natural parameter -1
__global__ void __launch_bounds__(64) walker_mu_reprice_kernel(const WalkerMuArgs A) {
    __shared__ int cnt[32];
    const int r = blockIdx.x, lane = threadIdx.x;
    if (r >= A.R) return;
    if (lane < 32) cnt[lane] = 0;
    __syncthreads();
    const uint8_t *occ = A.occ + (size_t)r * A.Npad;
    for (int k = 0; k < A.nsub; ++k)
        for (int a = lane; a < A.nact[k]; a += 64) atomicAdd(&cnt[k * 8 + (occ[A.sbase[k] + a] & 7)], 1);
    __syncthreads();
    if (lane == 0) {
        const double *ro = A.rows_old + (size_t)r * A.stride_old, *rn = A.rows_new + (size_t)r * A.stride_new;
        double w_old = 0.0, w_new = 0.0;
        for (int c = 0; c < 8 * A.nsub; ++c) {
            w_old += (double)cnt[c] * ro[c];
            w_new += (double)cnt[c] * rn[c];
        }
        A.features[(size_t)r * A.F + A.F - 1] += w_new - w_old;
        if (A.enthalpy) A.enthalpy[r] -= w_new - w_old;
    }
}
int smolmc_walker_mu_reprice(smolmc_handle *h, const double *rows_old, int stride_old, const double *rows_new, int stride_new,
                             double *features, int F, double *enthalpy) {
    const LeanParams &lp = h->lp;
    WalkerMuArgs A;
    memset(&A, 0, sizeof(A));
    A.occ = h->kp.occ; A.rows_old = rows_old; A.rows_new = rows_new; A.features = features; A.enthalpy = enthalpy;
    A.R = h->R; A.Npad = h->Npad; A.F = F; A.stride_old = stride_old; A.stride_new = stride_new;
    A.nsub = h->lean_multi() ? lp.m_nsub : 1;
    for (int k = 0; k < A.nsub; ++k) {
        A.sbase[k] = h->lean_multi() ? lp.m_sbase[k] : lp.sbase;
        A.nact[k] = h->lean_multi() ? lp.m_nact[k] : lp.nact;
    }
    hipLaunchKernelGGL(walker_mu_reprice_kernel, dim3((unsigned)h->R), dim3(64), 0, h->stream, A);
    HIPCHK(hipGetLastError());
    return 0;
}
