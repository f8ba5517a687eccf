// From a handle's runtime state to one kernel instantiation, and the launch every family shares.
//
// A family's launcher (the launch_*_nslot templates at the end of the kernel headers) computes a small runtime
// key, picks the matching entry of a compile-time variant list with first_match, and launches it with
// launch_timed.  A variant is a word of named flags (LV_*, TV_*, MV_*, WV_*, GV_* next to each kernel) from
// which the kernel's template arguments are derived in one place, so a new variant is one entry in one list.
//
// ORDER OF A VARIANT LIST.  The compiler emits a kernel where it is first referenced, so the order of a list
// is the order of its kernels in the code object.  The kernels call out-of-line helpers pc-relative: moving a
// kernel changes its bytes, and the isa_sha256 stamps of profiles/pmc_constants.json go stale.  The lists are
// therefore never sorted or regrouped; a new variant goes at the end of its list.  (`python -m smol_amd.codeobj`
// before and after a change shows whether a kernel moved.)
#pragma once
#include <type_traits>

// f(integral_constant<V>) for the first V of Vs that equals key; the last V is the `else` and takes every
// other key.  One LEFT fold, no recursion: the compiler expands it first to last, so the variants are referenced
// -- and their kernels emitted -- in list order (a right fold is expanded from its last element).
template <auto... Vs, typename Key, typename F> static int first_match(const Key key, F &&f) {
    int rc = 0;
    size_t left = sizeof...(Vs);
    (void)(... || (--left == 0 || key == Vs ? (rc = f(std::integral_constant<decltype(Vs), Vs>{}), true) : false));
    return rc;
}

// One kernel launch between the handle's two timing events; above 64 KiB the kernel's LDS limit is raised first.
template <typename... KArgs, typename... Args>
static int launch_timed(smolmc_handle *h, void (*kern)(KArgs...), dim3 grid, dim3 block, size_t lds, const Args &...args) {
    if (lds > 64 * 1024)
        HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIPCHK(hipEventRecord(h->ev0, h->stream));
    hipLaunchKernelGGL(kern, grid, block, lds, h->stream, args...);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev1, h->stream));
    h->timed = true;
    return 0;
}

// The (MM, STEP) pair of a handle on the lean layouts: f(mm, step) with both as integral constants.
template <typename F> static int with_mm_step(const smolmc_handle *h, F &&f) {
    return first_match<2, 3>(h->lean_mm, [&](auto mm) {
        return first_match<SMOLMC_STEP_SWAP, SMOLMC_STEP_FLIP>(h->cfg.step_type, [&](auto step) { return f(mm, step); });
    });
}
