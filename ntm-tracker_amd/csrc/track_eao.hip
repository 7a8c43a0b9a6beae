// The expected average overlap curve of the multi-start protocol, reduced on the device from the runs' table and overlap trace
// (contract: include/ntmtrack.h, NTK_MS_*, ntk_track_eao_curve).  Two kernels in fixed orders, no atomics: the same input gives
// the same bits.
#include "common.h"

namespace {

// N_F of a finished run: the failure's ordinal, or every scored frame; never more than the run's stretch of the trace holds.
__device__ __forceinline__ long long run_tracked(const double* row, long long room) {
    const double nf = row[NTK_MS_FAILED] != 0.0 ? row[NTK_MS_TRACKED] : row[NTK_MS_FRAMES];
    if (!(nf > 0) || room <= 0) return 0;
    return nf < (double)room ? (long long)nf : room;
}

}  // namespace

// (a) One 64-lane wavefront per run: prefix[first + i] = o_0 + ... + o_i for i < min(N_F, n_max), in chunks of 64 frames -- a
// wave scan (log-step shuffles) plus the total carried from the chunks before.  Nothing is stored beyond that.
__global__ __launch_bounds__(64) void track_eao_prefix_kernel(const double* __restrict__ table,
                                                              const long long* __restrict__ trace_first,
                                                              const double* __restrict__ trace, int n_max,
                                                              double* __restrict__ prefix) {
    const int run = blockIdx.x, lane = threadIdx.x;
    const long long first = trace_first[run], room = trace_first[run + 1] - first;
    long long m = run_tracked(table + (size_t)run * NTK_MS_HEAD, room);
    if (m > n_max) m = n_max;
    if (first < 0) return;
    double carry = 0.0;
    for (long long c = 0; c < m; c += 64) {             // m is uniform over the wave: every lane takes every shuffle
        const long long i = c + lane;
        double v = i < m ? trace[first + i] : 0.0;
        for (int d = 1; d < 64; d <<= 1) {
            const double u = __shfl_up(v, d, 64);
            if (lane >= d) v += u;
        }
        v += carry;
        if (i < m) prefix[first + i] = v;
        carry = __shfl(v, 63, 64);
    }
}

// (b) One thread per n = 1 ... n_max loops over the runs in run order: adjacent n read adjacent prefix entries of a run, the
// entry at a run's N_F is one address for all lanes beyond it, the table row is the same for all.
__global__ void track_eao_curve_kernel(const double* __restrict__ table, const long long* __restrict__ trace_first,
                                       const double* __restrict__ prefix, int n_runs, int n_max, double* __restrict__ curve) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x + 1;
    if (n > n_max) return;
    double acc = 0.0;
    long long members = 0;
    for (int run = 0; run < n_runs; ++run) {
        const double* row = table + (size_t)run * NTK_MS_HEAD;
        const double frames = row[NTK_MS_FRAMES];
        if (!(frames > 0)) continue;                                        // N = 0: the run takes part in nothing
        if (row[NTK_MS_FAILED] == 0.0 && frames < (double)n) continue;      // unfailed and shorter than n: not in S_n
        const long long first = trace_first[run];
        const long long nf = run_tracked(row, trace_first[run + 1] - first);
        const long long k = nf < n ? nf : n;
        if (k > 0 && first >= 0) acc += prefix[first + k - 1] / (double)n;
        members += 1;
    }
    curve[n - 1] = members ? acc / (double)members : __longlong_as_double(0x7ff8000000000000LL);
}

extern "C" int ntk_track_eao_curve(const double* table, const long long* trace_first, const double* trace, int n_runs, int n_max,
                                   double* prefix, double* curve, void* stream) {
    NTK_REQUIRE(table && trace_first && trace && prefix && curve, NTK_ERR_BAD_PTR, "ntk_track_eao_curve: null pointer");
    NTK_REQUIRE(n_runs > 0 && n_max > 0, NTK_ERR_BAD_SHAPE, "ntk_track_eao_curve: n_runs=%d n_max=%d", n_runs, n_max);
    track_eao_prefix_kernel<<<n_runs, 64, 0, (hipStream_t)stream>>>(table, trace_first, trace, n_max, prefix);
    NTK_CHECK_LAUNCH("ntk_track_eao_curve");
    track_eao_curve_kernel<<<(n_max + 63) / 64, 64, 0, (hipStream_t)stream>>>(table, trace_first, prefix, n_runs, n_max, curve);
    NTK_CHECK_LAUNCH("ntk_track_eao_curve");
    return NTK_OK;
}
