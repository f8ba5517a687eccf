"""The float32 thresholds of the straight rows swap kernels (smol_amd/csrc/rows_thresholds.h), probed on the device through
the test-only library (probe_sweeps.hip: the probe kernels call the very functions mc_lean_kernel calls).

The kernels take the two thresholds of a step from ONE word of its acceptance uniform: with m = w2 >> 8 the uniform
u = philox_u53(w2, w3) lies in [m 2^-24, (m + 1) 2^-24), and thr_hi / thr_lo are float32 evaluations of
T(m) = log2(m 2^-24) ln2 / -beta and of T(m + 1), widened by fast_eps and by a bound on the evaluation error.  Held here:

* the hardware log2 (v_log_f32) of every integer 1 .. 2^24, bare and scaled by 2^-24 (the form the thresholds use), against
  NumPy float64: the worst error in ulp of the result is PRINTED, must not exceed the figure recorded in the header
  (SMOLMC_ROWS_LOG2_MEASURED_ULP) and the widening constant W of the header must be at least twice it;
* enclosure: (double) thr_lo <= thr - fast_eps and (double) thr_hi >= thr + fast_eps with thr = log(u) * (1 / -beta), the
  float64 expression of the other kernels, evaluated in NumPy -- at 300 K, 2500 K and 40000 K, for a band of the headline
  handle's order (2^-18 eV: fast_eps = 2^-18 sum |w d|, with sum |w d| = 1 eV) and 1e-12, for every m < 2^16, every m
  within 1024 of a power of two, the ends, and 2^20 seeded random word pairs.  thr is monotone in u, so every m is checked
  at BOTH ends of its interval: (low bits of w2, w3) all zeros and all ones;
* tightness for m >= 2^20: thr_hi - thr_lo <= 2 fast_eps (1 + 2^-18) + 2e-6 |thr| + 1.001 kT ln(1 + 1/m).  The last term is
  the width of the interval itself, T(m) - T(m + 1): thresholds that do not read w3 cannot be closer than that (at most
  2^-20 kT here, 1.7e-7 |thr| at u = 1/2); the 2^-18 is the upward rounding of fast_eps to float32; 2e-6 covers twice the
  relative widening (W + 2) 2^-23 = 7.2e-7 of either threshold;
* a band of zero (SMOLMC_FAST_EPS_SCALE=0) gives -inf / +inf on every word."""

import ctypes as C
import functools

import numpy as np
import pytest

from tests import ewald_sweeps as es

pytestmark = pytest.mark.gpu

KB = 8.617333262e-5  # eV / K
TEMPS = (300.0, 2500.0, 40000.0)
FAST_EPS = (2.0 ** -18, 1e-12)
N24 = 1 << 24


def _probe():
    lib = es.load_probe()
    lib.smolmc_probe_rows_widen_ulp.restype, lib.smolmc_probe_rows_widen_ulp.argtypes = C.c_int, []
    lib.smolmc_probe_rows_measured_ulp.restype, lib.smolmc_probe_rows_measured_ulp.argtypes = C.c_double, []
    lib.smolmc_probe_rows_thresholds.restype = C.c_int
    lib.smolmc_probe_rows_thresholds.argtypes = [C.c_void_p, C.c_longlong, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
    lib.smolmc_probe_rows_log2.restype = C.c_int
    lib.smolmc_probe_rows_log2.argtypes = [C.c_uint32, C.c_longlong, C.c_int, C.c_void_p]
    return lib


def _thresholds(m, beta, fast_eps):
    """(thr_lo, thr_hi) of the words m << 8 on the device (the low bits of w2 do not enter)"""
    import torch

    lib = _probe()
    w2 = torch.from_numpy((m.astype(np.int64) << 8).astype(np.uint32).view(np.int32)).to("cuda:0")
    lo = torch.empty(len(m), dtype=torch.float32, device="cuda:0")
    hi = torch.empty_like(lo)
    torch.cuda.synchronize()
    rc = lib.smolmc_probe_rows_thresholds(w2.data_ptr(), len(m), float(beta), float(fast_eps), lo.data_ptr(), hi.data_ptr())
    assert rc == 0, rc
    return lo.cpu().numpy(), hi.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _words():
    """m of every tested word: all m < 2^16, within 1024 of every power of two, the ends; then 2^20 random pairs"""
    near = [np.arange(max(0, (1 << k) - 1024), min(N24, (1 << k) + 1025)) for k in range(25)]
    m = np.unique(np.concatenate([np.arange(1 << 16), np.array([0, N24 - 1])] + near)).astype(np.int64)
    rng = np.random.default_rng(20240607)
    w2 = rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64)
    w3 = rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64)
    for a in (m, w2, w3):
        a.setflags(write=False)
    return m, w2, w3


def _u53(w2, w3):
    """philox_u53 (philox.h) in NumPy"""
    k = ((w2.astype(np.uint64) >> np.uint64(5)) << np.uint64(26)) | (w3.astype(np.uint64) >> np.uint64(6))
    return k.astype(np.float64) * 2.0 ** -53


@pytest.mark.parametrize("scaled", [0, 1], ids=["integer", "scaled-by-2^-24"])
def test_hardware_log2_of_every_integer(scaled):
    import torch

    lib = _probe()
    out = torch.empty(N24, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    assert lib.smolmc_probe_rows_log2(1, N24, scaled, out.data_ptr()) == 0
    got = out.cpu().numpy().astype(np.float64)
    ref = np.log2(np.arange(1, N24 + 1, dtype=np.float64)) - (24.0 if scaled else 0.0)
    zero = ref == 0.0
    assert np.all(got[zero] == 0.0)  # log2(1) is exact: the threshold of m + 1 = 2^24 is -fast_eps, nothing else
    ulp = np.spacing(np.abs(ref[~zero]).astype(np.float32)).astype(np.float64)
    err = np.abs(got[~zero] - ref[~zero]) / ulp
    k = int(np.argmax(err))
    worst = float(err[k])
    W, rec = lib.smolmc_probe_rows_widen_ulp(), lib.smolmc_probe_rows_measured_ulp()
    print(f"[rows thresholds] v_log_f32 over 1 .. 2^24 ({'m 2^-24' if scaled else 'm'}): worst error {worst:.4f} ulp at "
          f"m = {int(np.flatnonzero(~zero)[k]) + 1}; recorded {rec}, widening constant W = {W}")
    assert worst <= rec, (worst, rec)
    assert W >= 2.0 * worst, (W, worst)


def _thr(u, beta):
    with np.errstate(divide="ignore"):
        return np.log(u) * (1.0 / -beta)


@pytest.mark.parametrize("fast_eps", FAST_EPS)
@pytest.mark.parametrize("T", TEMPS)
def test_thresholds_enclose_the_float64_band(T, fast_eps):
    beta = 1.0 / (KB * T)
    m, rw2, rw3 = _words()
    lo, hi = _thresholds(m, beta, fast_eps)
    lo, hi = lo.astype(np.float64), hi.astype(np.float64)
    assert not np.any(np.isnan(lo)) and not np.any(np.isnan(hi))
    # both ends of every interval: the remaining 8 + 32 bits all zeros (thr largest), all ones (thr smallest)
    w2 = m.astype(np.uint64) << np.uint64(8)
    for low, w3, what in ((0, 0, "zeros"), (0xFF, 0xFFFFFFFF, "ones")):
        thr = _thr(_u53(w2 | np.uint64(low), np.full(len(m), w3, np.uint64)), beta)
        bad = ~((lo <= thr - fast_eps) & (hi >= thr + fast_eps))
        assert not bad.any(), (what, T, fast_eps, m[bad][:5], lo[bad][:5], thr[bad][:5], hi[bad][:5])
    assert hi[0] == np.inf and m[0] == 0  # u = 0: the float64 rule accepts everything, no finite threshold is above it
    # random pairs
    rm = (rw2 >> np.uint64(8)).astype(np.int64)
    rlo, rhi = _thresholds(rm, beta, fast_eps)
    thr = _thr(_u53(rw2, rw3), beta)
    bad = ~((rlo.astype(np.float64) <= thr - fast_eps) & (rhi.astype(np.float64) >= thr + fast_eps))
    assert not bad.any(), (T, fast_eps, rm[bad][:5])
    # tightness, m >= 2^20
    kT = 1.0 / beta
    for mm, l, h in ((m, lo, hi), (rm, rlo.astype(np.float64), rhi.astype(np.float64))):
        big = mm >= (1 << 20)
        assert big.sum() > 1000
        mb = mm[big].astype(np.float64)
        thr_min = np.abs(_thr((mb + 1.0) * 2.0 ** -24, beta))  # the smallest |thr| of the interval
        bound = 2.0 * fast_eps * (1.0 + 2.0 ** -18) + 2e-6 * thr_min + 1.001 * kT * np.log1p(1.0 / mb)
        width = h[big] - l[big]
        k = int(np.argmax(width / bound))
        print(f"[rows thresholds] T = {T}, fast_eps = {fast_eps:.3g}: largest width / bound {width[k] / bound[k]:.4f} at m = {int(mb[k])}")
        assert np.all(width <= bound), (T, fast_eps, int(mb[k]), width[k], bound[k])


@pytest.mark.parametrize("T", TEMPS)
def test_a_band_of_zero_selects_the_exact_path_on_every_word(T):
    m, rw2, _ = _words()
    for mm in (m, (rw2 >> np.uint64(8)).astype(np.int64)):
        lo, hi = _thresholds(mm, 1.0 / (KB * T), 0.0)
        assert np.all(lo == -np.inf) and np.all(hi == np.inf)
