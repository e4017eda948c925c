// select_harness.hip — test-only driver for lightkurve_amd/csrc/block_select.hpp (never linked into liblkhip.so).
// tests/select_harness.py compiles it into a shared library of its own; tests/test_block_select_gpu.py calls it.
// Every launch runs G independent problems, one workgroup each, and reports per problem the results AND the route word: the
// OR of (1 << SelRoute id) over every LK_SEL_ROUTE() the workgroup passed.  The hooks sit on workgroup-uniform branches, so
// thread 0 alone keeps the word (in LDS, touched by no other thread) and stores it with an ordinary store at the end.
// The entry points take host pointers, validate every precondition the header states (they never launch a problem the
// header does not define), do their own hipMalloc / hipMemcpy / launch / hipDeviceSynchronize and return the HIP error
// code (0 = ok, -1 = a precondition was violated, nothing launched).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

__shared__ unsigned int selh_route_word;
__device__ __forceinline__ void selh_route_mark(int id) {
    if (threadIdx.x == 0) selh_route_word |= 1u << id;
}
#define LK_SEL_ROUTE(id) selh_route_mark((int)(id))
#include "block_select.hpp"

using namespace lk;
static_assert(SEL_R_COUNT <= 32, "the route word is 32 bits");

namespace {

struct Prob {          // numpy dtype in tests/select_harness.py (48 bytes)
    long long off;     // first value of the problem in the value / mask arrays
    long long count;   // number of kept values (the host wrapper fills it in from the mask)
    long long k;       // rank (select ops); qa (hist op)
    int n;             // values in the problem
    int aux;           // want_next (sampled select); qb (hist op)
    double guess;      // block_median_near guess; lo of the bracket (hist op)
    double width;      // block_median_near width; hi of the bracket (hist op)
};
static_assert(sizeof(Prob) == 48, "Prob layout");

enum { OP_KTH = 0, OP_MEDIAN, OP_SAMPLED, OP_MEDIAN_SAMPLED, OP_NEAR, OP_HIST, OP_N };
constexpr int ND = 8, NI = 4;   // doubles / int64 per problem in the outputs

// counts the calls of the side functor and keeps the range of the `lo` it was handed
struct CountSide {
    long long *calls;
    double *lo_min, *lo_max;
    __device__ __forceinline__ void operator()(int, double, double lo) const {
        ++*calls;
        *lo_min = fmin(*lo_min, lo);
        *lo_max = fmax(*lo_max, lo);
    }
};

__global__ __launch_bounds__(1024) void selh_select_kernel(int op, int cap, const double *v, const unsigned char *mask,
                                                            const Prob *probs, double *outd, long long *outi,
                                                            unsigned int *routes) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long lds[];
    const int tid = threadIdx.x, nt = blockDim.x;
    if (tid == 0) selh_route_word = 0u;
    unsigned long long *sh = lds;
    double *cand = reinterpret_cast<double *>(lds + max(nt, 264));
    const Prob p = probs[blockIdx.x];
    const double *x = v + p.off;
    const unsigned char *mk = mask ? mask + p.off : nullptr;
    auto val = [&](int i) { return x[i]; };
    auto keep = [&](int i) { return mk ? mk[i] != 0 : true; };
    double r = 0.0, nxt = 0.0, spacing = 0.0, r2 = 0.0;
    bool flag = false;
    long long calls = 0, untouched = 1;
    double lo_min = INFINITY, lo_max = -INFINITY;
    const CountSide side{&calls, &lo_min, &lo_max};
    if (op == OP_KTH) {
        r = block_select_kth(p.n, p.k, val, keep, sh);
    } else if (op == OP_MEDIAN) {
        r = block_median(p.n, p.count, val, keep, sh);
    } else if (op == OP_SAMPLED) {
        r = block_select_sampled(p.n, p.count, p.k, val, keep, sh, cand, cap, p.aux != 0, &nxt, &spacing, side, &flag);
    } else if (op == OP_MEDIAN_SAMPLED) {
        r = block_median_sampled(p.n, p.count, val, keep, sh, cand, cap, &spacing, side, &flag);
    } else if (op == OP_NEAR) {
        r = block_median_near(p.n, p.count, val, keep, p.guess, p.width, sh, cand, cap, &flag, side);
    } else if (op == OP_HIST) {
        for (int i = tid; i < p.n; i += nt) cand[i] = x[i];
        __syncthreads();
        flag = lds_hist_select(cand, p.n, cap, (int)p.k, p.aux, p.guess, p.width, sh, &r, &r2);
        __syncthreads();
        long long same = 0;   // the candidates, bit for bit where they were
        for (int i = tid; i < p.n; i += nt) same += __double_as_longlong(cand[i]) == __double_as_longlong(x[i]) ? 1 : 0;
        untouched = block_count_dyn(same, reinterpret_cast<long long *>(sh)) == (long long)p.n ? 1 : 0;
        nxt = r2;
    }
    // the side functor's tallies, reduced over the workgroup with the plainest code there is
    __syncthreads();
    long long *shl = reinterpret_cast<long long *>(sh);
    double *shd = reinterpret_cast<double *>(sh);
    shl[tid] = calls;
    __syncthreads();
    long long all_calls = 0;
    for (int i = 0; i < nt; ++i) all_calls += shl[i];
    __syncthreads();
    shd[tid] = lo_min;
    __syncthreads();
    double all_min = INFINITY;
    for (int i = 0; i < nt; ++i) all_min = fmin(all_min, shd[i]);
    __syncthreads();
    shd[tid] = lo_max;
    __syncthreads();
    double all_max = -INFINITY;
    for (int i = 0; i < nt; ++i) all_max = fmax(all_max, shd[i]);
    __syncthreads();
    // every thread must hold the same result: thread 0 writes it, the last thread's copy goes next to it
    double *od = outd + (size_t)blockIdx.x * ND;
    long long *oi = outi + (size_t)blockIdx.x * NI;
    if (tid == nt - 1) {
        od[5] = r;
        od[6] = nxt;
    }
    if (tid == 0) {
        od[0] = r;
        od[1] = nxt;
        od[2] = spacing;
        od[3] = all_min;
        od[4] = all_max;
        od[7] = 0.0;
        oi[0] = flag ? 1 : 0;
        oi[1] = all_calls;
        oi[2] = untouched;
        oi[3] = 0;
        routes[blockIdx.x] = selh_route_word;
    }
}

// S keys per problem sorted in LDS
__global__ __launch_bounds__(1024) void selh_sort_kernel(int S, const unsigned long long *in, unsigned long long *out) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long lds[];
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int i = tid; i < S; i += nt) lds[i] = in[(size_t)blockIdx.x * S + i];
    __syncthreads();
    lds_bitonic_sort(lds, S);
    __syncthreads();
    for (int i = tid; i < S; i += nt) out[(size_t)blockIdx.x * S + i] = lds[i];
}

// one value per thread through the scan and the four reductions; every thread writes what IT got back
enum { RED_EXSCAN = 0, RED_SUM_DYN, RED_SUM_FAST, RED_COUNT_DYN, RED_COUNT_FAST, RED_N };
__global__ __launch_bounds__(1024) void selh_reduce_kernel(int op, const double *xd, const long long *xi, double *outd,
                                                            long long *outi, long long *tot) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long lds[];
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (op == RED_EXSCAN) {
        int t = 0;
        outi[g] = block_exscan_int((int)xi[g], reinterpret_cast<int *>(lds), &t);
        tot[g] = t;
    } else if (op == RED_SUM_DYN) {
        outd[g] = block_sum_dyn(xd[g], reinterpret_cast<double *>(lds));
    } else if (op == RED_SUM_FAST) {
        outd[g] = block_sum_fast(xd[g], reinterpret_cast<double *>(lds));
    } else if (op == RED_COUNT_DYN) {
        outi[g] = block_count_dyn(xi[g], reinterpret_cast<long long *>(lds));
    } else if (op == RED_COUNT_FAST) {
        outi[g] = block_count_fast(xi[g], reinterpret_cast<long long *>(lds));
    }
}

__global__ void selh_sortable_kernel(int n, const double *x, unsigned long long *key, double *back) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        key[i] = f64_sortable(x[i]);
        back[i] = f64_from_sortable(key[i]);
    }
}

// device buffers of one call, freed on every way out
struct Bufs {
    std::vector<void *> p;
    ~Bufs() {
        for (void *q : p) (void)hipFree(q);
    }
    hipError_t in(void **d, const void *h, size_t bytes) {
        hipError_t e = hipMalloc(d, bytes ? bytes : 8);
        if (e != hipSuccess) return e;
        p.push_back(*d);
        return bytes ? hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice) : hipSuccess;
    }
    hipError_t out(void **d, size_t bytes) {
        hipError_t e = hipMalloc(d, bytes ? bytes : 8);
        if (e != hipSuccess) return e;
        p.push_back(*d);
        return hipMemset(*d, 0xff, bytes ? bytes : 8);
    }
};
#define SELH_CHECK(x)                        \
    do {                                     \
        const hipError_t e_ = (x);           \
        if (e_ != hipSuccess) return (int)e_; \
    } while (0)

bool block_ok(int nt) { return nt >= 64 && nt <= 1024 && nt % 64 == 0; }

int finish() {
    SELH_CHECK(hipGetLastError());
    SELH_CHECK(hipDeviceSynchronize());
    return 0;
}

}  // namespace

extern "C" {

int selh_route_count() { return (int)SEL_R_COUNT; }
int selh_prob_size() { return (int)sizeof(Prob); }

// op in OP_*; nt threads per workgroup; G problems over `total` values (mask: NULL = keep all).  outd: G x 8 doubles,
// outi: G x 4 int64, routes: G uint32.
int selh_select(int op, int nt, int cap, int G, long long total, const double *v, const unsigned char *mask,
                const void *probs_v, double *outd, long long *outi, unsigned int *routes) {
    const Prob *probs = static_cast<const Prob *>(probs_v);
    if (op < 0 || op >= OP_N || !block_ok(nt) || G <= 0 || cap < 0 || total < 0) return -1;
    const size_t lds_bytes = ((size_t)(nt > 264 ? nt : 264) + (size_t)cap + 2) * 8;
    if (lds_bytes + 64 > 64 * 1024) return -1;
    long long seen_off = -1, seen_n = -1, c = 0;   // (consecutive problems often share one data set: counted once)
    for (int g = 0; g < G; ++g) {
        const Prob &p = probs[g];
        if (p.n < 0 || p.off < 0 || p.off + p.n > total) return -1;
        if (p.off != seen_off || p.n != seen_n) {
            c = 0;
            for (int i = 0; i < p.n; ++i) {
                if (mask ? mask[p.off + i] != 0 : true) {
                    if (v[p.off + i] != v[p.off + i]) return -1;   // kept NaN: outside the header's contract
                    ++c;
                }
            }
            seen_off = p.off;
            seen_n = p.n;
        }
        if (c != p.count) return -1;
        if ((op == OP_KTH || op == OP_SAMPLED) && !(p.k >= 0 && p.k < c)) return -1;
        if (op == OP_HIST) {   // ranks among n <= cap candidates strictly inside (lo, hi); -1 = not wanted
            if (mask || p.n > cap || p.k < -1 || p.k >= p.n || p.aux < -1 || p.aux >= p.n) return -1;
            for (int i = 0; i < p.n; ++i)
                if (!(v[p.off + i] > p.guess && v[p.off + i] < p.width)) return -1;
        }
    }
    Bufs b;
    double *dv, *dd;
    unsigned char *dm = nullptr;
    Prob *dp;
    long long *di;
    unsigned int *dr;
    SELH_CHECK(b.in((void **)&dv, v, (size_t)total * 8));
    if (mask) SELH_CHECK(b.in((void **)&dm, mask, (size_t)total));
    SELH_CHECK(b.in((void **)&dp, probs, (size_t)G * sizeof(Prob)));
    SELH_CHECK(b.out((void **)&dd, (size_t)G * ND * 8));
    SELH_CHECK(b.out((void **)&di, (size_t)G * NI * 8));
    SELH_CHECK(b.out((void **)&dr, (size_t)G * 4));
    hipLaunchKernelGGL(selh_select_kernel, dim3(G), dim3(nt), lds_bytes, 0, op, cap, dv, dm, dp, dd, di, dr);
    if (int rc = finish()) return rc;
    SELH_CHECK(hipMemcpy(outd, dd, (size_t)G * ND * 8, hipMemcpyDeviceToHost));
    SELH_CHECK(hipMemcpy(outi, di, (size_t)G * NI * 8, hipMemcpyDeviceToHost));
    SELH_CHECK(hipMemcpy(routes, dr, (size_t)G * 4, hipMemcpyDeviceToHost));
    return 0;
}

// G problems of S = 2^m keys each
int selh_sort(int nt, int S, int G, const unsigned long long *in, unsigned long long *out) {
    if (!block_ok(nt) || G <= 0 || S < 2 || S > 8192 || (S & (S - 1)) != 0) return -1;
    const size_t lds_bytes = (size_t)S * 8;
    if (lds_bytes + 64 > 64 * 1024)   // the 8192-key sort: raise the kernel's dynamic-LDS limit as lk::want_lds does
        SELH_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(selh_sort_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    Bufs b;
    unsigned long long *di, *dout;
    SELH_CHECK(b.in((void **)&di, in, (size_t)G * S * 8));
    SELH_CHECK(b.out((void **)&dout, (size_t)G * S * 8));
    hipLaunchKernelGGL(selh_sort_kernel, dim3(G), dim3(nt), lds_bytes, 0, S, di, dout);
    if (int rc = finish()) return rc;
    SELH_CHECK(hipMemcpy(out, dout, (size_t)G * S * 8, hipMemcpyDeviceToHost));
    return 0;
}

// G workgroups of nt threads, one input per thread (xd for the sums, xi for the scan and the counts); outputs per thread
int selh_reduce(int op, int nt, int G, const double *xd, const long long *xi, double *outd, long long *outi,
                long long *tot) {
    if (op < 0 || op >= RED_N || !block_ok(nt) || G <= 0) return -1;
    const size_t N = (size_t)G * nt;
    if (op == RED_EXSCAN)
        for (size_t i = 0; i < N; ++i)
            if (xi[i] < 0 || xi[i] > (1 << 20)) return -1;   // nt x 2^20 stays inside an int
    Bufs b;
    double *dxd, *dod;
    long long *dxi, *doi, *dt;
    SELH_CHECK(b.in((void **)&dxd, xd, N * 8));
    SELH_CHECK(b.in((void **)&dxi, xi, N * 8));
    SELH_CHECK(b.out((void **)&dod, N * 8));
    SELH_CHECK(b.out((void **)&doi, N * 8));
    SELH_CHECK(b.out((void **)&dt, N * 8));
    hipLaunchKernelGGL(selh_reduce_kernel, dim3(G), dim3(nt), (size_t)(nt > 264 ? nt : 264) * 8, 0, op, dxd, dxi, dod, doi, dt);
    if (int rc = finish()) return rc;
    SELH_CHECK(hipMemcpy(outd, dod, N * 8, hipMemcpyDeviceToHost));
    SELH_CHECK(hipMemcpy(outi, doi, N * 8, hipMemcpyDeviceToHost));
    SELH_CHECK(hipMemcpy(tot, dt, N * 8, hipMemcpyDeviceToHost));
    return 0;
}

int selh_sortable(int n, const double *x, unsigned long long *key, double *back) {
    if (n <= 0) return -1;
    Bufs b;
    double *dx, *db;
    unsigned long long *dk;
    SELH_CHECK(b.in((void **)&dx, x, (size_t)n * 8));
    SELH_CHECK(b.out((void **)&dk, (size_t)n * 8));
    SELH_CHECK(b.out((void **)&db, (size_t)n * 8));
    hipLaunchKernelGGL(selh_sortable_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, n, dx, dk, db);
    if (int rc = finish()) return rc;
    SELH_CHECK(hipMemcpy(key, dk, (size_t)n * 8, hipMemcpyDeviceToHost));
    SELH_CHECK(hipMemcpy(back, db, (size_t)n * 8, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
