// fold_phase.hpp — the phase and the cycle of one cadence, shared by fold.hip (fold + sort), foldbin.hip (fold + bin, no sort)
// and river.hip (cycle x phase images).  The translation units are compiled with the same flags, so the expressions below round
// the same way in all of them and the fused kernels see the bits fold_kernel writes.
#pragma once
#include <hip/hip_runtime.h>

namespace lk {

// numpy's `%` for floats: the result takes the divisor's sign
__device__ __forceinline__ double np_mod(double a, double b) {
    double m = fmod(a, b);
    if (m != 0.0) {
        if ((b < 0.0) != (m < 0.0)) m += b;
    } else {
        m = copysign(0.0, b);
    }
    return m;
}

// The per-target constants of astropy's TimeSeries.fold (timeseries/sampled.py:230-233): wrap_phase defaults to P/2 (or 0.5
// when normalising); in phase units it and epoch_phase are multiplied by P.
struct FoldPar {
    double P, ep, eph, shift;
    int normalize;
};

__device__ __forceinline__ FoldPar fold_par(double P, double epoch_time, double epoch_phase, double wrap_phase, int normalize_phase) {
    FoldPar f;
    f.P = P;
    f.ep = epoch_time;
    const double wrap = normalize_phase ? wrap_phase * P : wrap_phase;
    f.eph = normalize_phase ? epoch_phase * P : epoch_phase;
    f.shift = P - wrap;
    f.normalize = normalize_phase;
    return f;
}

// phase = ((t - epoch) + epoch_phase + (P - wrap)) % P - (P - wrap), divided by P when normalising
__device__ __forceinline__ double fold_phase(const FoldPar &f, double t) {
    const double rel = ((t - f.ep) + f.eph) + f.shift;
    double ph = np_mod(rel, f.P) - f.shift;
    if (f.normalize) ph = ph / f.P;
    return ph;
}

// FoldedLightCurve.cycle before the minimum is taken off (foldbin.hip's odd / even cycles, river.hip's rows)
__device__ __forceinline__ double fb_cycle(double t, double e, double P) { return floor((t - (e - P / 2.0)) / P); }

}  // namespace lk
