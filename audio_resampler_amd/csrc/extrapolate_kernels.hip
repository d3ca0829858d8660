// extrapolate_kernels.hip — LPC end-point extrapolation on the device (EXTRAPOLATE_ENDPOINTS, artamdExtrapolateBatchDevice).
//
// A 4-coefficient linear predictor is fitted to a run of known samples by coordinate descent with a halving step (at most
// 100,000 probes, step floor 3 / 2^22), its reflection (PARCOR) coefficients are clamped to +-0.9999, degenerate fits fall back
// to "repeat the last sample" or "silence", and the predictor is then run past the newest sample (or, on the time-reversed run,
// before the oldest).  The float / double mixing follows the reference's extrapolator expression by expression, so the samples
// are bit-identical to it.  This file is built with -ffp-contract=off and keeps f32 subnormals: both are load-bearing.
//
// One workgroup of one wave per run.  The fit is a chain of probes, each depending on the last accepted one, and the reference
// decides every probe on two serial left-to-right double sums ("down" and "up") over the run.  Here:
//   - the residual of the current predictor and every term (resid[k] -+ x[k+3-w]*step)^2, for all four coefficients w at once,
//     are computed across the lanes, each term in the reference's operation order (so each term is the reference's, bit for bit);
//   - the eight sums are summed in any order (per lane, then a butterfly across the wave).  All terms are >= 0, so the serial sum
//     S and the parallel one P of the same n terms both lie within gamma(n-1) * sum of the exact sum: |S - P| <= K * P with
//     K = (4 n + 8) u (u = 2^-53), a bound that also covers the rounding of the interval ends;
//   - a comparison the reference makes (down < best, up < best, down < up) is decided from the intervals when they prove it.
//     Otherwise (ties, a non-finite sum, an overlap) both sides are summed serially in the reference's order and compared as
//     the reference compares them;
//   - `best` is the serial value of the accepted sum.  It is kept as its parallel value plus what it was made of (the residual
//     array of its probe, the coefficient, the sign and the step), so that its exact value is computed only when a later
//     comparison needs it.  The residual arrays ping-pong in LDS: a new probe never overwrites the array `best` refers to.
// The once-per-fit sums (energy of the values and of the deltas, the error of the final predictor) are serial.  Every lane
// computes the same values, so control flow is uniform.
#include <hip/hip_runtime.h>
#include <cmath>
#include "art_internal.h"

#define XO 4                                     // predictor order (reference NCOEFFS)
#define X_PROBES 100000                          // reference MAXLOOPS
#define X_LANES 64
#define X_PER_LANE ((ARTAMD_EXTRAPOLATE_MAX_KNOWN - XO + X_LANES - 1) / X_LANES)

namespace {

struct XFit {
    const art_s *x;                              // LDS, the run in fit order (oldest first)
    double *resid;                               // LDS, [2][MAX_KNOWN - XO]
    int evals;
    double K;                                    // relative bound |serial - parallel| <= K * parallel
};

// one quantity the reference compares: a sum over the residual array `buf` of terms (resid[k] + sign * x[k+3-w] * step)^2
struct XSum {
    double v;                                    // serial value when exact, else the parallel value
    bool exact;
    int buf, w;
    bool down;                                   // term (resid - d)^2 (true) or (resid + d)^2
    double step;
};

__device__ double serial_sum (const XFit &f, const XSum &s)
{
    const double *r = f.resid + (size_t) s.buf * (ARTAMD_EXTRAPOLATE_MAX_KNOWN - XO);
    double acc = 0.0;
    for (int k = 0; k < f.evals; ++k) {
        const double d = f.x [k + XO - s.w - 1] * s.step;
        acc += s.down ? (r [k] - d) * (r [k] - d) : (r [k] + d) * (r [k] + d);
    }
    return acc;
}

__device__ void make_exact (const XFit &f, XSum &s)
{
    if (!s.exact) { s.v = serial_sum (f, s); s.exact = true; }
}

// the interval that holds the serial value; false when none can be given (a non-finite or huge parallel value)
__device__ bool interval (const XFit &f, const XSum &s, double &lo, double &hi)
{
    if (s.exact) { lo = hi = s.v; return true; }
    if (!(s.v >= 0.0 && s.v <= 1.0e300)) return false;
    const double e = s.v * f.K;
    lo = s.v - e; hi = s.v + e;
    return true;
}

// the reference's `a < b` on the serial values
__device__ bool less (const XFit &f, XSum &a, XSum &b)
{
    double alo, ahi, blo, bhi;
    if (interval (f, a, alo, ahi) && interval (f, b, blo, bhi)) {
        if (ahi < blo) return true;
        if (alo >= bhi) return false;
    }
    make_exact (f, a); make_exact (f, b);
    return a.v < b.v;
}

__device__ double wave_sum (double v)
{
    for (int m = X_LANES / 2; m > 0; m >>= 1) v += __shfl_xor (v, m, X_LANES);     // (commutative: every lane gets the same bits)
    return v;
}

__device__ void reflection_from_predictor (const double *lpc, double *refl)
{
    double cur [XO], next [XO];
    for (int i = 0; i < XO; ++i) cur [i] = lpc [i];
    for (int m = XO - 1; m >= 0; --m) {
        refl [m] = cur [m];
        double den = 1.0 - (refl [m] * refl [m]);
        if (fabs (den) < 1e-6) {
            refl [m] = refl [m] < 0.0 ? -0.9999995 : 0.9999995;
            den = 1.0 - (refl [m] * refl [m]);
        }
        for (int i = 0; i < m; ++i) next [i] = (cur [i] - refl [m] * cur [m - i - 1]) / den;
        for (int i = 0; i < m; ++i) cur [i] = next [i];
    }
}

__device__ void predictor_from_reflection (const double *refl, double *lpc)
{
    for (int i = 0; i < XO; ++i) {
        lpc [i] = refl [i];
        for (int j = 0; j < i / 2; ++j) {
            const double held = lpc [j];
            lpc [j] += refl [i] * lpc [i - 1 - j];
            lpc [i - 1 - j] += refl [i] * held;
        }
        if (i & 1) lpc [i >> 1] += lpc [i >> 1] * refl [i];
    }
}

// fit coeffs[XO] so that x[n] ~ -(sum_c coeffs[XO-1-c] * x[n-XO+c]); every lane returns the same coefficients
__device__ void fit_predictor (XFit &f, float *coeffs)
{
    const int lane = threadIdx.x, evals = f.evals;
    const art_s *x = f.x;
    double energy = 0.0, delta_energy = 0.0, step = 3.0 / (1 << 4);
    int probes = 0, accepted = 0;

    for (int c = 0; c < XO; ++c) coeffs [c] = 0.0f;

    for (int i = 0; i < evals; ++i) {
        const art_s d = x [i + XO] - x [i + XO - 1];
        delta_energy += d * d;
        energy += x [i + XO] * x [i + XO];
    }
    if (energy == 0.0) return;

    XSum best = { energy, true, 0, 0, true, 0.0 };
    int cur = 0;

    // (a lazy best is a sum of terms >= 0, none NaN: its serial value is > 0 exactly when its parallel one is)
    while (best.v > 0.0 && probes < X_PROBES) {
        if (!best.exact) cur = best.buf ^ 1;
        double *resid = f.resid + (size_t) cur * (ARTAMD_EXTRAPOLATE_MAX_KNOWN - XO);
        double pd [XO], pu [XO];
        for (int w = 0; w < XO; ++w) pd [w] = pu [w] = 0.0;

        #pragma unroll
        for (int j = 0; j < X_PER_LANE; ++j) {
            const int k = lane + j * X_LANES;
            if (k < evals) {
                double acc = 0.0;
                for (int c = 0; c < XO; ++c) acc += coeffs [XO - c - 1] * x [k + c];
                const double r = acc + x [k + XO];
                resid [k] = r;
                #pragma unroll
                for (int w = 0; w < XO; ++w) {
                    const double d = x [k + XO - w - 1] * step;
                    pd [w] += (r - d) * (r - d);
                    pu [w] += (r + d) * (r + d);
                }
            }
        }
        for (int w = 0; w < XO; ++w) { pd [w] = wave_sum (pd [w]); pu [w] = wave_sum (pu [w]); }
        __syncthreads ();                        // (the serial sums read the whole residual array)

        int which;
        for (which = 0; probes++, which < XO; which++) {
            XSum down = { pd [which], false, cur, which, true, step };
            XSum up = { pu [which], false, cur, which, false, step };
            if (less (f, down, best) || less (f, up, best)) {
                if (less (f, down, up)) { best = down; coeffs [which] -= step; }
                else                    { best = up;   coeffs [which] += step; }
                accepted++;
                break;
            }
        }

        if (which == XO) {
            if (step > 3.0 / (1 << 22)) step *= 0.5;
            else break;
        }
        __syncthreads ();                        // (the next probe rewrites a residual array the serial sums may have read)
    }

    if (accepted) {
        double lpc [XO], refl [XO];
        int clamped = 0;
        for (int i = 0; i < XO; ++i) lpc [i] = coeffs [i];
        reflection_from_predictor (lpc, refl);
        for (int i = 0; i < XO; ++i)
            if (fabs (refl [i]) > 0.9999) { refl [i] = refl [i] < 0.0 ? -0.9999 : 0.9999; clamped++; }
        if (clamped) {
            predictor_from_reflection (refl, lpc);
            for (int i = 0; i < XO; ++i) coeffs [i] = lpc [i];
        }
    }

    double err = 0.0;
    for (int k = 0; k < evals; ++k) {
        double acc = 0.0;
        for (int c = 0; c < XO; ++c) acc += coeffs [XO - c - 1] * x [k + c];
        err += (acc + x [k + XO]) * (acc + x [k + XO]);
    }

    if (delta_energy < err && delta_energy < energy) {
        for (int c = 0; c < XO; ++c) coeffs [c] = 0.0f;
        coeffs [0] = -1.0f;
    }
    else if (energy <= err)
        for (int c = 0; c < XO; ++c) coeffs [c] = 0.0f;
}

__global__ __launch_bounds__ (X_LANES) void extrapolate_kernel (const ArtExtrapRun *runs)
{
    __shared__ art_s x [ARTAMD_EXTRAPOLATE_MAX_KNOWN];
    __shared__ double resid [2 * (ARTAMD_EXTRAPOLATE_MAX_KNOWN - XO)];
    const ArtExtrapRun r = runs [blockIdx.x];
    const int count = r.n [0] + r.n [1], lane = threadIdx.x;

    for (int i = lane; i < count; i += X_LANES) {         // fit order: oldest first (backward: the time-reversed run)
        const int j = r.backward ? count - 1 - i : i;
        x [i] = j < r.n [0] ? r.src [0][(long) j * r.stride [0]] : r.src [1][(long)(j - r.n [0]) * r.stride [1]];
    }
    __syncthreads ();

    XFit f = { x, resid, count - XO, (4.0 * (count - XO) + 8.0) * 0x1p-53 };
    float coeffs [XO];
    fit_predictor (f, coeffs);

    if (lane == 0) {                             // the prediction recurrence: each new sample feeds the next
        art_s tail [XO];
        for (int c = 0; c < XO; ++c) tail [c] = x [count - XO + c];
        for (long i = 0; i < r.extras; ++i) {
            double acc = 0.0;
            for (int c = 0; c < XO; ++c) acc += tail [c] * coeffs [XO - c - 1];
            const art_s v = -acc;
            r.out [i * r.out_stride] = v;
            for (int c = 0; c < XO - 1; ++c) tail [c] = tail [c + 1];
            tail [XO - 1] = v;
        }
    }
}

// the launch table of the calling thread (device memory kept across calls; see arthip_ingest_batch)
struct ExtrapTable { void *d; size_t cap; int device; hipEvent_t ev; hipStream_t last; bool used; };

}  // namespace

extern "C" int arthip_extrapolate (const ArtExtrapRun *runs, int n, void *stream)
{
    static thread_local ExtrapTable t = { nullptr, 0, -1, nullptr, nullptr, false };
    hipStream_t st = (hipStream_t) stream;
    const size_t bytes = sizeof (ArtExtrapRun) * (size_t) n;
    int device = 0;
    if (n <= 0) return 0;
    if (hipGetDevice (&device) != hipSuccess) return -1;
    if (t.device != device || bytes > t.cap) {
        if (t.used) (void) hipEventSynchronize (t.ev);
        if (t.d) (void) hipFree (t.d);
        if (t.ev && t.device != device) { (void) hipEventDestroy (t.ev); t.ev = nullptr; }
        t.d = nullptr; t.cap = 0; t.used = false; t.device = device;
        if (!t.ev && hipEventCreateWithFlags (&t.ev, hipEventDisableTiming) != hipSuccess) { t.ev = nullptr; return -1; }
        const size_t cap = bytes * 2 > 4096 ? bytes * 2 : 4096;
        if (hipMalloc (&t.d, cap) != hipSuccess) { t.d = nullptr; return -1; }
        t.cap = cap;
    }
    if (t.used && t.last != st && hipStreamWaitEvent (st, t.ev, 0) != hipSuccess) return -1;
    if (arthip_table_upload (runs, bytes, t.d, st)) return -1;
    hipLaunchKernelGGL (extrapolate_kernel, dim3 ((unsigned int) n), dim3 (X_LANES), 0, st, (const ArtExtrapRun *) t.d);
    if (hipGetLastError () != hipSuccess) return -1;
    if (hipEventRecord (t.ev, st) != hipSuccess) { t.used = false; return hipStreamSynchronize (st) == hipSuccess ? 0 : -1; }
    t.last = st; t.used = true;
    return 0;
}
