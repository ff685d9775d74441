// probe_gather.hip -- what bounds a k_wind-shaped gather on MI355X?  (diagnostic, not product)
//
// k_wind walks, for every coastal-band cell, the nz-level pressure column of a caller-owned (lon, lat, lev)
// array: runs of band cells along longitude (28 cells = 224 bytes on average inside a 64-cell segment) times
// nz planes 39 MB apart.  This program times that access pattern with the run length, its alignment, the
// order of the walk and the loads in flight as parameters, next to a plain stream of the same bytes, and a
// k_scan-shaped stream (two arrays in, one out).
//
//   hipcc -O3 --offload-arch=gfx950 tools/probe_gather.hip -o tools/_build/probe_gather && tools/_build/probe_gather
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>

#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

// a wave takes segments gw, gw+NW, ...; segment s starts at cell s*stride + shift(s); its first `act` lanes walk
template <int UN, bool LEVEL_MAJOR>
__global__ __launch_bounds__(256) void k_gather(const double *__restrict__ p, size_t plane, int nz, int nseg, int act,
                                                int stride, int misalign, double *__restrict__ out) {
    const int gw = (blockIdx.x * 256 + threadIdx.x) >> 6, nw = (gridDim.x * 256) >> 6;
    const int lane = threadIdx.x & 63;
    auto cell_of = [&](int s) { return (size_t)s * stride + (misalign ? (s * 7) % 16 : 0) + lane; };
    if (!LEVEL_MAJOR) {
        for (int s = gw; s < nseg; s += nw) {
            const size_t cell = cell_of(s);
            if (lane < act) {
                double best = 1e300;
                int lev = 0;
                for (int k0 = 0; k0 < nz; k0 += UN) {
                    double d[UN];
#pragma unroll
                    for (int q = 0; q < UN; ++q) d[q] = __builtin_nontemporal_load(p + cell + (size_t)(k0 + q < nz ? k0 + q : nz - 1) * plane);
#pragma unroll
                    for (int q = 0; q < UN; ++q) { const double a = fabs(d[q] - 70000.0); if (a < best) { best = a; lev = k0 + q; } }
                }
                out[cell] = best + lev;
            }
        }
    } else {
        // the wave's (up to 4) segments advance through the levels together: at any time the chip touches few planes
        constexpr int MS = 4;
        for (int base = gw; base < nseg; base += MS * nw) {
            double best[MS];
            int lev[MS];
#pragma unroll
            for (int j = 0; j < MS; ++j) { best[j] = 1e300; lev[j] = 0; }
            for (int k0 = 0; k0 < nz; k0 += UN) {
#pragma unroll
                for (int j = 0; j < MS; ++j) {
                    const int s = base + j * nw;
                    if (s < nseg && lane < act) {
                        const size_t cell = cell_of(s);
                        double d[UN];
#pragma unroll
                        for (int q = 0; q < UN; ++q) d[q] = __builtin_nontemporal_load(p + cell + (size_t)(k0 + q < nz ? k0 + q : nz - 1) * plane);
#pragma unroll
                        for (int q = 0; q < UN; ++q) { const double a = fabs(d[q] - 70000.0); if (a < best[j]) { best[j] = a; lev[j] = k0 + q; } }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < MS; ++j) {
                const int s = base + j * nw;
                if (s < nseg && lane < act) out[cell_of(s)] = best[j] + lev[j];
            }
        }
    }
}

// Two (LV = 2) or four (LV = 4) levels per 16-byte load: a lane takes an aligned PAIR of cells of the segment (double2),
// the 64 / LV lanes of one group cover 128 / LV cells of one level and group h = lane / (64 / LV) loads level LV*i + h
// in instruction i -- the lines of k_gather<UN, false>, 1 / LV of its load instructions.  UN: instructions per batch.
// A run that starts at an odd cell begins (and may end) in a pair that holds one band cell.  Each lane keeps (best, lev)
// of its two cells over the levels of its group; the groups combine at the end (smaller best wins; where neither is
// smaller the lower level), then lane j takes cell j's result from lane j >> 1.  Same output as k_gather.
typedef double probe_d2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void pair_combine(double &best, int &lev, int mask) {
    const double ob = __shfl_xor(best, mask);
    const int ol = __shfl_xor(lev, mask);
    if (ob < best || (!(best < ob) && ol < lev)) { best = ob; lev = ol; }
}
template <int UN, int LV>
__global__ __launch_bounds__(256) void k_gather_pair(const double *__restrict__ p, size_t plane, int nz, int nseg, int act,
                                                     int stride, int misalign, double *__restrict__ out) {
    constexpr int NP = 64 / LV;                          // lanes (pairs) per level
    const int gw = (blockIdx.x * 256 + threadIdx.x) >> 6, nw = (gridDim.x * 256) >> 6;
    const int lane = threadIdx.x & 63, m = lane & (NP - 1), h = lane / NP;
    const int ni = (nz + LV - 1) / LV;
    for (int s = gw; s < nseg; s += nw) {
        const size_t b = (size_t)s * stride + (misalign ? (s * 7) % 16 : 0), a = b & ~(size_t)1;
        const bool on = a + 2 * m < b + act;             // the pair holds a cell of the run
        double best0 = 1e300, best1 = 1e300;
        int lev0 = h ? 0x7fffffff : 0, lev1 = lev0;
        if (on) {
            const double *pc = p + a + 2 * m;
            for (int i0 = 0; i0 < ni; i0 += UN) {
                probe_d2 d[UN];
#pragma unroll
                for (int q = 0; q < UN; ++q) {
                    const int k = LV * (i0 + q) + h;
                    d[q] = __builtin_nontemporal_load((const probe_d2 *)(pc + (size_t)(k < nz ? k : nz - 1) * plane));
                }
#pragma unroll
                for (int q = 0; q < UN; ++q) {
                    const int k = LV * (i0 + q) + h;
                    const double a0 = fabs(d[q].x - 70000.0), a1 = fabs(d[q].y - 70000.0);
                    if (k < nz && a0 < best0) { best0 = a0; lev0 = k; }
                    if (k < nz && a1 < best1) { best1 = a1; lev1 = k; }
                }
            }
        }
#pragma unroll
        for (int mask = 32; mask >= NP; mask >>= 1) { pair_combine(best0, lev0, mask); pair_combine(best1, lev1, mask); }
        const double e0 = __shfl(best0, lane >> 1), e1 = __shfl(best1, lane >> 1);
        const int f0 = __shfl(lev0, lane >> 1), f1 = __shfl(lev1, lane >> 1);
        const size_t cell = a + lane;
        if (lane < 2 * NP && cell >= b && cell < b + act) out[cell] = (lane & 1) ? e1 + f1 : e0 + f0;
    }
}

// a wave takes MS ADJACENT segments (neighbours along longitude: the same pages of every plane) and walks them together,
// UN levels of each in flight: per level one page of the plane serves MS loads of the wave
template <int UN, int MS>
__global__ __launch_bounds__(256) void k_gather_adj(const double *__restrict__ p, size_t plane, int nz, int nseg, int act,
                                                    int stride, int misalign, double *__restrict__ out) {
    const int gw = (blockIdx.x * 256 + threadIdx.x) >> 6, nw = (gridDim.x * 256) >> 6;
    const int lane = threadIdx.x & 63;
    auto cell_of = [&](int s) { return (size_t)s * stride + (misalign ? (s * 7) % 16 : 0) + lane; };
    for (int base = gw * MS; base < nseg; base += MS * nw) {
        double best[MS];
        int lev[MS];
        size_t cell[MS];
#pragma unroll
        for (int j = 0; j < MS; ++j) { best[j] = 1e300; lev[j] = 0; cell[j] = cell_of(base + j < nseg ? base + j : nseg - 1); }
        if (lane < act) {
            for (int k0 = 0; k0 < nz; k0 += UN) {
                double d[MS][UN];
#pragma unroll
                for (int q = 0; q < UN; ++q)
#pragma unroll
                    for (int j = 0; j < MS; ++j) d[j][q] = __builtin_nontemporal_load(p + cell[j] + (size_t)(k0 + q < nz ? k0 + q : nz - 1) * plane);
#pragma unroll
                for (int j = 0; j < MS; ++j)
#pragma unroll
                    for (int q = 0; q < UN; ++q) { const double a = fabs(d[j][q] - 70000.0); if (a < best[j]) { best[j] = a; lev[j] = k0 + q; } }
            }
#pragma unroll
            for (int j = 0; j < MS; ++j) if (base + j < nseg) out[cell[j]] = best[j] + lev[j];
        }
    }
}

// k_scan-shaped stream: read a and b, write c where a lane-dependent predicate holds (90 % of the cells)
__global__ __launch_bounds__(1024) void k_stream2in1out(const double *__restrict__ a, const double *__restrict__ b,
                                                        double *__restrict__ c, size_t n, int wr) {
    const size_t stride = (size_t)gridDim.x * 1024;
    double acc = 0;
    for (size_t i = (size_t)blockIdx.x * 1024 + threadIdx.x; i < n; i += 4 * stride) {
        double x[4], y[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { const size_t j = i + q * stride < n ? i + q * stride : i; x[q] = a[j]; y[q] = b[j]; }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            acc += x[q];
            if (wr && i + q * stride < n && !(fabs(y[q]) <= 180.0)) c[i + q * stride] = 0.0;
        }
    }
    if (acc == 1.2345) c[0] = acc;
}

static double median(std::vector<float> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

int main() {
    CHK(hipSetDevice(0));
    hipDeviceProp_t pr;
    CHK(hipGetDeviceProperties(&pr, 0));
    const int ncu = pr.multiProcessorCount;
    hipStream_t s1;
    CHK(hipStreamCreateWithFlags(&s1, hipStreamNonBlocking));
    hipEvent_t e0, e1;
    CHK(hipEventCreate(&e0));
    CHK(hipEventCreate(&e1));
    const int nz = 56;
    const size_t plane = (size_t)2560 * 1920;
    double *p, *out;
    CHK(hipMalloc(&p, plane * nz * sizeof(double)));
    CHK(hipMemset(p, 0, plane * nz * sizeof(double)));
    CHK(hipMalloc(&out, plane * sizeof(double)));
    auto timeit = [&](auto fn) {
        std::vector<float> t;
        for (int r = 0; r < 9; ++r) {
            CHK(hipEventRecord(e0, s1));
            fn();
            CHK(hipEventRecord(e1, s1));
            CHK(hipEventSynchronize(e1));
            float ms;
            CHK(hipEventElapsedTime(&ms, e0, e1));
            t.push_back(ms);
        }
        return median(t) * 1e3;
    };
    struct Mmm { double mn, md, mx; };
    auto timeit3 = [&](auto fn) {                     // min, median, max of 9 repetitions, us
        std::vector<float> t;
        for (int r = 0; r < 9; ++r) {
            CHK(hipEventRecord(e0, s1));
            fn();
            CHK(hipEventRecord(e1, s1));
            CHK(hipEventSynchronize(e1));
            float ms;
            CHK(hipEventElapsedTime(&ms, e0, e1));
            t.push_back(ms);
        }
        std::sort(t.begin(), t.end());
        return Mmm{t.front() * 1e3, t[t.size() / 2] * 1e3, t.back() * 1e3};
    };
    struct Case { const char *name; int nseg, act, stride, misalign; };
    // all cases move ~214 MB of algorithmic bytes except where noted
    const Case cases[] = {
        {"28 lanes, runs start anywhere (k_wind-like)      ", 17085, 28, 287, 1},
        {"28 lanes, runs start on a line boundary          ", 17085, 28, 272, 0},
        {"32 lanes = 2 whole lines                         ", 14950, 32, 320, 0},
        {"16 lanes = 1 whole line                          ", 29900, 16, 160, 0},
        {"64 lanes = 4 whole lines (512 B pieces)          ", 7475, 64, 640, 0},
        {"64 lanes, segments contiguous (stream by planes) ", 7475, 64, 64, 0},
    };
    for (const Case &c : cases) {
        const double alg = (double)c.nseg * c.act * nz * 8;
        // lines touched per piece
        double lines = 0;
        for (int s = 0; s < c.nseg; ++s) {
            const size_t b0 = ((size_t)s * c.stride + (c.misalign ? (s * 7) % 16 : 0)) * 8, b1 = b0 + c.act * 8 - 1;
            lines += (double)(b1 / 128 - b0 / 128 + 1);
        }
        const double fetched = lines * 128 * nz;
        printf("%s alg %.0f MB, lines %.0f MB\n", c.name, alg / 1e6, fetched / 1e6);
        for (int wgs : {4, 8}) {
            const dim3 g(ncu * wgs), b(256);
            const double t8 = timeit([&] { hipLaunchKernelGGL((k_gather<8, false>), g, b, 0, s1, p, plane, nz, c.nseg, c.act, c.stride, c.misalign, out); });
            const double t28 = timeit([&] { hipLaunchKernelGGL((k_gather<28, false>), g, b, 0, s1, p, plane, nz, c.nseg, c.act, c.stride, c.misalign, out); });
            const double t56 = timeit([&] { hipLaunchKernelGGL((k_gather<56, false>), g, b, 0, s1, p, plane, nz, c.nseg, c.act, c.stride, c.misalign, out); });
            const double l8 = timeit([&] { hipLaunchKernelGGL((k_gather<8, true>), g, b, 0, s1, p, plane, nz, c.nseg, c.act, c.stride, c.misalign, out); });
            const double l14 = timeit([&] { hipLaunchKernelGGL((k_gather<14, true>), g, b, 0, s1, p, plane, nz, c.nseg, c.act, c.stride, c.misalign, out); });
            printf("   %d WG/CU: cell-major un8 %.1f us (%.0f GB/s of lines)  un28 %.1f  un56 %.1f | level-major un8 %.1f (%.0f GB/s)  un14 %.1f\n",
                   wgs, t8, fetched / t8 / 1e3, t28, t56, l8, fetched / l8 / 1e3, l14);
            const double a24 = timeit([&] { hipLaunchKernelGGL((k_gather_adj<4, 2>), g, b, 0, s1, p, plane, nz, c.nseg, c.act, c.stride, c.misalign, out); });
            const double a44 = timeit([&] { hipLaunchKernelGGL((k_gather_adj<4, 4>), g, b, 0, s1, p, plane, nz, c.nseg, c.act, c.stride, c.misalign, out); });
            const double a28 = timeit([&] { hipLaunchKernelGGL((k_gather_adj<2, 8>), g, b, 0, s1, p, plane, nz, c.nseg, c.act, c.stride, c.misalign, out); });
            const double a82 = timeit([&] { hipLaunchKernelGGL((k_gather_adj<8, 2>), g, b, 0, s1, p, plane, nz, c.nseg, c.act, c.stride, c.misalign, out); });
            printf("              adjacent segments walked together (levels x segments in flight): 4x2 %.1f us  4x4 %.1f (%.0f GB/s of lines)  2x8 %.1f  8x2 %.1f\n",
                   a24, a44, fetched / a44 / 1e3, a28, a82);
#define PROBE_ARGS g, b, 0, s1, p, plane, nz, c.nseg, c.act, c.stride, c.misalign, out
            const Mmm r8 = timeit3([&] { hipLaunchKernelGGL((k_gather<8, false>), PROBE_ARGS); });
            const Mmm p4 = timeit3([&] { hipLaunchKernelGGL((k_gather_pair<4, 2>), PROBE_ARGS); });
            const Mmm p7 = timeit3([&] { hipLaunchKernelGGL((k_gather_pair<7, 2>), PROBE_ARGS); });
            const Mmm p14 = timeit3([&] { hipLaunchKernelGGL((k_gather_pair<14, 2>), PROBE_ARGS); });
            printf("              min/median/max of 9: cell-major un8 %.1f/%.1f/%.1f us | pairs, two levels per 16-byte load: un4 %.1f/%.1f/%.1f  un7 %.1f/%.1f/%.1f  un14 %.1f/%.1f/%.1f\n",
                   r8.mn, r8.md, r8.mx, p4.mn, p4.md, p4.mx, p7.mn, p7.md, p7.mx, p14.mn, p14.md, p14.mx);
            if (c.act <= 32 - c.misalign) {          // four levels per load: 16 pairs = 32 cells hold the run (recorded only)
                const Mmm q4 = timeit3([&] { hipLaunchKernelGGL((k_gather_pair<4, 4>), PROBE_ARGS); });
                const Mmm q7 = timeit3([&] { hipLaunchKernelGGL((k_gather_pair<7, 4>), PROBE_ARGS); });
                const Mmm q14 = timeit3([&] { hipLaunchKernelGGL((k_gather_pair<14, 4>), PROBE_ARGS); });
                printf("              pairs, four levels per load: un4 %.1f/%.1f/%.1f  un7 %.1f/%.1f/%.1f  un14 %.1f/%.1f/%.1f\n",
                       q4.mn, q4.md, q4.mx, q7.mn, q7.md, q7.mx, q14.mn, q14.md, q14.mx);
            }
#undef PROBE_ARGS
        }
    }
    // k_scan-shaped stream
    {
        double *a, *b, *c;
        const size_t n = plane;
        CHK(hipMalloc(&a, n * 8 * 8));
        CHK(hipMalloc(&b, n * 8 * 8));
        CHK(hipMalloc(&c, n * 8 * 8));
        CHK(hipMemset(a, 0, n * 8 * 8));
        CHK(hipMemset(b, 0x7f, n * 8 * 8));      // |b| huge: every cell is written
        CHK(hipMemset(c, 0, n * 8 * 8));
        int rot = 0;
        for (int wr : {0, 1})
            for (int wgs : {1, 2}) {
                const double t = timeit([&] {
                    rot = (rot + 1) % 8;          // rotate through 8 copies: nothing is served from the caches
                    hipLaunchKernelGGL(k_stream2in1out, dim3(ncu * wgs), dim3(1024), 0, s1, a + rot * n, b + rot * n, c + rot * n, n, wr);
                });
                printf("stream 2 in%s, %d x 1024 threads per CU: %.1f us, %.0f GB/s\n", wr ? " 1 out" : "      ", wgs, t,
                       (double)n * 8 * (2 + wr) / t / 1e3);
            }
    }
    printf("done\n");
    return 0;
}
