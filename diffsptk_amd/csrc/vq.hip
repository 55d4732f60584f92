// Vector quantisation and codebook design (include/diffsptk_amd.h, section a23): the nearest-codeword search of VectorQuantization,
// vq.py:110-125, the lookup of InverseVectorQuantization, ivq.py:63-67, and one iteration of LindeBuzoGrayAlgorithm.forward,
// lbg.py:214-285.  (There: a (B, K) distance matrix per DataLoader batch, histc, scatter_add_ and a masked division.)
//   search   one thread per vector; a tile of vectors in LDS (row stride L | 1: conflict-free), the codebook staged through LDS
//            DSA_VQ_CHUNK codewords at a time, as float64 and four to a group, so K has no ceiling.  Four codewords per pass over a
//            vector: one LDS read of x and two 16-byte broadcast reads per four differences.  The differences and their squares are float64 whatever x's type: the assignment is that of exact
//            arithmetic apart from ties closer than float64 rounding; on a tie the first index wins.  The minimal distances are
//            summed per workgroup (fixed order); `total`, when asked for, by one workgroup of a second kernel.
//   accum    per codeword the count and the float64 sum of its vectors.  Grid (chunk of codewords, segment of T), four waves per
//            workgroup: wave g takes the runs g, g + 4, ... of 64 vectors of its segment -- one read of 64 indices, then the vectors
//            that fall into the chunk in the order of t --, lane j column j, and adds into its own LDS image of the chunk: every LDS
//            cell belongs to one thread: no atomics, the same bits every run.  The four images are added in
//            wave order into the workspace's segment.
//   update   per codeword the segments' counts and sums (four interleaved runs of the segments, each in order, added in run order) and
//            the centroid rounded to float32 into the caller's pending buffer; then one workgroup of a second kernel forms the three
//            numbers the host reads per iteration (distance, clusters below the minimum, first largest cluster).
//   lookup   xq = codebook[indices].
//   vjp      gx = g_xq + g_loss 2 (x - xq) / n.
#include "common.h"

#include <limits>

namespace dsa {
namespace {

// dsa_last_kernel() of the entries: [entry][dtype]
enum { VQ_SEARCH = 0, VQ_ACCUM = 1, VQ_UPDATE = 2, VQ_LOOKUP = 3, VQ_VJP = 4 };
const char* const kVqRoutes[5][2] = {
    {"vq_search_f32", "vq_search_f64"}, {"vq_accum_f32", "vq_accum_f64"}, {"vq_update", "vq_update"},
    {"vq_lookup_f32", "vq_lookup_f64"}, {"vq_vjp_f32", "vq_vjp_f64"},
};

constexpr int VQ_ACCUM_WAVES = 4;          // images of a chunk per workgroup of the accumulation
constexpr int VQ_ACCUM_LDS_BYTES = 65536;  // what its images may take: no raised limit needed
constexpr int VQ_FILL_WAVES = 4096;        // waves below which T is split into segments: four per SIMD of 256 compute units
constexpr int VQ_SEGMENT_MIN = 256;        // vectors per segment at least

inline int64_t vq_accum_chunk(int64_t K, int64_t L)
{
    const int64_t fit = VQ_ACCUM_LDS_BYTES / (VQ_ACCUM_WAVES * (8 * L + 4));
    return K < fit ? K : fit;
}
inline int vq_accum_segments(int64_t T, int64_t K, int64_t L)
{
    const int64_t KC = vq_accum_chunk(K, L), waves = VQ_ACCUM_WAVES * ((K + KC - 1) / KC);   // the waves of one segment
    if (waves >= VQ_FILL_WAVES) return 1;
    int64_t s = (VQ_FILL_WAVES + waves - 1) / waves;
    const int64_t by_t = (T + VQ_SEGMENT_MIN - 1) / VQ_SEGMENT_MIN;
    s = s < by_t ? s : by_t;
    s = s < DSA_VQ_MAX_SEGMENTS ? s : DSA_VQ_MAX_SEGMENTS;
    return (int)(s < 1 ? 1 : s);
}

// ---------------------------------------------------------------------------------------------------------------- search
template <typename T>
__global__ __launch_bounds__(DSA_VQ_TILE_BYTES / sizeof(T)) void vq_search_kernel(const T* __restrict__ x, const float* __restrict__ cb, long Tn,
                                                                                  int K, int L, int64_t* __restrict__ idx, T* __restrict__ xq,
                                                                                  double* __restrict__ partial)
{
    constexpr int TILE = DSA_VQ_TILE_BYTES / sizeof(T);
    extern __shared__ __align__(16) unsigned char vq_lds[];
    __shared__ double red[TILE / 64];
    const int S = L | 1;
    T* xs = reinterpret_cast<T*>(vq_lds);   // (TILE, S) vectors
    // (DSA_VQ_CHUNK / 4, L, 4) codewords as float64, four to a group: element j of a group's four codewords is two 16-byte reads
    double* cd = reinterpret_cast<double*>(xs + TILE * S);
    const int tid = threadIdx.x;
    const long t0 = (long)blockIdx.x * TILE, t = t0 + tid;
    const long rows = Tn - t0 < TILE ? Tn - t0 : TILE;
    for (long e = tid; e < rows * L; e += TILE) xs[(e / L) * S + e % L] = x[t0 * L + e];
    const bool live = t < Tn;
    const T* xt = xs + tid * S;
    double best = dsa_inf<double>();
    int arg = 0;
    for (int k0 = 0; k0 < K; k0 += DSA_VQ_CHUNK) {
        const int kn = K - k0 < DSA_VQ_CHUNK ? K - k0 : DSA_VQ_CHUNK, kn4 = (kn + 3) & ~3;
        __syncthreads();   // the chunk before this one has been read out of LDS (and, at k0 = 0, the tile is in)
        for (int e = tid; e < kn4 * L; e += TILE) {   // a group's places past the end repeat the last codeword and are not compared
            const int q = e / L, j = e % L, src = q < kn ? q : kn - 1;
            cd[((q >> 2) * L + j) * 4 + (q & 3)] = (double)cb[(long)(k0 + src) * L + j];
        }
        __syncthreads();
        if (!live) continue;
        for (int q = 0; q < kn; q += 4) {   // four codewords per pass over the vector
            const double2* cg = reinterpret_cast<const double2*>(cd + (q >> 2) * L * 4);
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
            for (int j = 0; j < L; ++j) {
                const double v = (double)xt[j];
                const double2 a = cg[2 * j], b = cg[2 * j + 1];
                const double d0 = v - a.x, d1 = v - a.y, d2 = v - b.x, d3 = v - b.y;
                s0 += d0 * d0;
                s1 += d1 * d1;
                s2 += d2 * d2;
                s3 += d3 * d3;
            }
            if (s0 < best) {   // strictly: on a tie the first index stays
                best = s0;
                arg = k0 + q;
            }
            if (q + 1 < kn && s1 < best) {
                best = s1;
                arg = k0 + q + 1;
            }
            if (q + 2 < kn && s2 < best) {
                best = s2;
                arg = k0 + q + 2;
            }
            if (q + 3 < kn && s3 < best) {
                best = s3;
                arg = k0 + q + 3;
            }
        }
    }
    double mine = 0.0;
    if (live) {
        idx[t] = arg;
        if (xq)
            for (int j = 0; j < L; ++j) xq[t * L + j] = (T)cb[(long)arg * L + j];
        mine = best;
    }
    const double all = block_sum<double>(mine, red);
    if (tid == 0) partial[blockIdx.x] = all;
}

template <typename T>
__global__ __launch_bounds__(256) void vq_total_kernel(const double* __restrict__ partial, long n, double scale, T* __restrict__ total)
{
    __shared__ double red[4];
    double s = 0.0;
    for (long i = threadIdx.x; i < n; i += 256) s += partial[i];
    const double all = block_sum<double>(s, red);
    if (threadIdx.x == 0) total[0] = (T)(all * scale);
}

// ---------------------------------------------------------------------------------------------------------------- accumulation
// sums[(s K + k) L + j] = sum over segment s of x[t,j] where idx[t] = k; counts[s K + k] the number of those t
template <typename T>
__global__ __launch_bounds__(64 * VQ_ACCUM_WAVES) void vq_accum_kernel(const T* __restrict__ x, const int64_t* __restrict__ idx, long Tn, int K,
                                                                       int L, long seglen, int KC, double* __restrict__ sums,
                                                                       int64_t* __restrict__ counts)
{
    extern __shared__ __align__(16) unsigned char vq_lds[];
    constexpr int NT = 64 * VQ_ACCUM_WAVES;
    double* acc = reinterpret_cast<double*>(vq_lds);                   // (VQ_ACCUM_WAVES, KC, L)
    int* cnt = reinterpret_cast<int*>(acc + VQ_ACCUM_WAVES * KC * L);   // (VQ_ACCUM_WAVES, KC)
    const int tid = threadIdx.x, lane = tid & 63, g = tid >> 6, seg = blockIdx.y;
    const int k0 = blockIdx.x * KC, kn = K - k0 < KC ? K - k0 : KC;
    for (int e = tid; e < VQ_ACCUM_WAVES * KC * L; e += NT) acc[e] = 0.0;
    for (int e = tid; e < VQ_ACCUM_WAVES * KC; e += NT) cnt[e] = 0;
    __syncthreads();
    const long tbeg = seg * seglen, tend = tbeg + seglen < Tn ? tbeg + seglen : Tn;
    double* mine = acc + g * KC * L;
    int* mc = cnt + g * KC;
    const bool col = lane < L;
    for (long tb = tbeg + 64 * g; tb < tend; tb += 64 * VQ_ACCUM_WAVES) {   // 64 indices per read; the wave then walks its hits in the order of t
        const long t = tb + lane;
        const long kk = t < tend ? (long)idx[t] - k0 : -1;
        const int mine_k = kk >= 0 && kk < kn ? (int)kk : -1;
        unsigned long long hits = __ballot(mine_k >= 0);   // the same in every lane: the loops below are uniform
        while (hits) {   // four vectors in flight
            int src[4], k[4];
            T v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                src[u] = hits ? __ffsll((long long)hits) - 1 : -1;
                hits &= hits - (hits != 0);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                k[u] = __shfl(mine_k, src[u] < 0 ? 0 : src[u], 64);
                v[u] = col && src[u] >= 0 ? x[(tb + src[u]) * L + lane] : (T)0;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (src[u] >= 0) {
                    if (col) mine[k[u] * L + lane] += (double)v[u];
                    if (lane == 0) mc[k[u]] += 1;
                }
        }
    }
    __syncthreads();
    const long img = (long)KC * L;
    for (int e = tid; e < kn * L; e += NT) sums[((long)seg * K + k0) * L + e] = ((acc[e] + acc[img + e]) + acc[2 * img + e]) + acc[3 * img + e];
    for (int e = tid; e < kn; e += NT) counts[(long)seg * K + k0 + e] = (int64_t)cnt[e] + cnt[KC + e] + cnt[2 * KC + e] + cnt[3 * KC + e];
}
static_assert(VQ_ACCUM_WAVES == 4, "vq_accum_kernel adds four images");

// ---------------------------------------------------------------------------------------------------------------- update
// one workgroup per codeword: wave g adds the segments g, g + 4, ... in order, the four runs are then added in wave order
__global__ __launch_bounds__(256) void vq_update_kernel(const double* __restrict__ sums, const int64_t* __restrict__ counts, int nseg, int K, int L,
                                                        long min_data, int64_t* __restrict__ n_data, float* __restrict__ pending)
{
    __shared__ long cnt[256];
    __shared__ double run[4][64];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, g = tid >> 6;
    long c = 0;
    for (int s = tid; s < nseg; s += 256) c += counts[(long)s * K + k];
    cnt[tid] = c;
    double a = 0.0;
    if (lane < L) {
#pragma unroll 8
        for (int s = g; s < nseg; s += 4) a += sums[((long)s * K + k) * L + lane];
    }
    run[g][lane] = a;
    __syncthreads();
    long n = 0;
    for (int i = 0; i < (nseg < 256 ? nseg : 256); ++i) n += cnt[i];   // integers: any order gives the same number
    if (tid == 0) n_data[k] = n;
    if (tid < L) {
        const double total = ((run[0][tid] + run[1][tid]) + run[2][tid]) + run[3][tid];
        pending[(long)k * L + tid] = n >= min_data ? (float)(total / (double)n) : 0.0f;   // min_data >= 1: never 0 / 0
    }
}

// the iteration's three numbers, by one workgroup
__global__ __launch_bounds__(256) void vq_readback_kernel(const int64_t* __restrict__ n_data, int K, const double* __restrict__ partial, long npartial,
                                                          double Tn, long min_data, double* __restrict__ readback)
{
    __shared__ double red[4];
    __shared__ long top_n[256];
    __shared__ int top_k[256], below[256];
    const int tid = threadIdx.x;
    double d = 0.0;
    for (long i = tid; i < npartial; i += 256) d += partial[i];
    const double all = block_sum<double>(d, red);
    long bn = -1;
    int bk = 0, small = 0;
    for (int kk = tid; kk < K; kk += 256) {
        const long c = n_data[kk];
        small += c < min_data;
        if (c > bn) {   // ascending kk: the first of equal counts stays
            bn = c;
            bk = kk;
        }
    }
    top_n[tid] = bn;
    top_k[tid] = bk;
    below[tid] = small;
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < 256; ++i) {
            small += below[i];
            if (top_n[i] > bn || (top_n[i] == bn && top_k[i] < bk)) {
                bn = top_n[i];
                bk = top_k[i];
            }
        }
        readback[0] = all / Tn;
        readback[1] = (double)small;
        readback[2] = (double)bk;
    }
}

// ---------------------------------------------------------------------------------------------------------------- lookup, adjoint
template <typename T>
__global__ __launch_bounds__(256) void vq_lookup_kernel(const int64_t* __restrict__ idx, const float* __restrict__ cb, long n, int K, int L,
                                                        T* __restrict__ xq)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const long k = idx[e / L];
    xq[e] = k >= 0 && k < K ? (T)cb[k * L + e % L] : std::numeric_limits<T>::quiet_NaN();
}

template <typename T>
__global__ __launch_bounds__(256) void vq_vjp_kernel(const T* __restrict__ g_xq, const T* __restrict__ g_loss, const T* __restrict__ x,
                                                     const T* __restrict__ xq, long n, T* __restrict__ gx)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    T g = g_xq ? g_xq[e] : (T)0;
    if (g_loss) g += g_loss[0] * (T)2 * (x[e] - xq[e]) / (T)n;
    gx[e] = g;
}

// ---------------------------------------------------------------------------------------------------------------- host
int vq_check(const char*& route, int entry, int64_t T, int64_t K, int64_t L, int32_t dtype)
{
    if (!(T >= 0 && K >= 1 && L >= 1)) return fail(DSA_ERR_INVALID_ARGUMENT, "vq: invalid sizes");
    if (dtype != DSA_F32 && dtype != DSA_F64) return fail(DSA_ERR_INVALID_ARGUMENT, "vq: unknown dtype");
    if (L > DSA_VQ_MAX_LENGTH && entry != VQ_LOOKUP)
        return fail(DSA_ERR_INVALID_ARGUMENT, "vq: vectors longer than DSA_VQ_MAX_LENGTH (64 elements) are not supported");
    // every tensor's byte offset is an int64, every launch dimension an int32: T L, K L, 256 K (L + 1), T / 128 workgroups
    if (K > (int64_t)1 << 24 || L > (int64_t)1 << 24 || T > INT64_MAX / 16 / L || T / (DSA_VQ_TILE_BYTES / 8) >= INT32_MAX ||
        T * L / 256 >= INT32_MAX)
        return fail(DSA_ERR_INVALID_ARGUMENT, "vq: invalid sizes");
    route = kVqRoutes[entry][dtype == DSA_F64];
    return DSA_OK;
}

template <typename T>
int vq_search(const void* x, const void* cb, int64_t Tn, int64_t K, int64_t L, void* idx, void* xq, void* partial, void* total, double scale,
              hipStream_t st)
{
    constexpr int TILE = DSA_VQ_TILE_BYTES / sizeof(T);
    constexpr int MAX_LDS = DSA_VQ_TILE_BYTES * (DSA_VQ_MAX_LENGTH | 1) + DSA_VQ_CHUNK * DSA_VQ_MAX_LENGTH * 8;
    const int64_t blocks = (Tn + TILE - 1) / TILE;
    const size_t lds = (size_t)TILE * (L | 1) * sizeof(T) + (size_t)DSA_VQ_CHUNK * L * 8;
    if (int rc = launch_lds<vq_search_kernel<T>>(MAX_LDS, "vq: cannot raise the dynamic LDS limit", dim3((unsigned)blocks), dim3(TILE), lds, st,
                                                 (const T*)x, (const float*)cb, (long)Tn, (int)K, (int)L, (int64_t*)idx, (T*)xq, (double*)partial))
        return rc;
    if (total)
        hipLaunchKernelGGL((vq_total_kernel<T>), dim3(1), dim3(256), 0, st, (const double*)partial, (long)blocks, scale, (T*)total);
    return DSA_OK;
}

template <typename T>
int vq_accum(const void* x, const void* idx, int64_t Tn, int64_t K, int64_t L, void* ws, hipStream_t st)
{
    const int nseg = vq_accum_segments(Tn, K, L);
    const int64_t KC = vq_accum_chunk(K, L);
    const long seglen = (long)((Tn + nseg - 1) / nseg);
    double* sums = (double*)ws;
    int64_t* counts = (int64_t*)(sums + (int64_t)nseg * K * L);
    const size_t lds = (size_t)VQ_ACCUM_WAVES * KC * (8 * L + 4);
    hipLaunchKernelGGL((vq_accum_kernel<T>), dim3((unsigned)((K + KC - 1) / KC), (unsigned)nseg), dim3(64 * VQ_ACCUM_WAVES), lds, st, (const T*)x,
                       (const int64_t*)idx, (long)Tn, (int)K, (int)L, seglen, (int)KC, sums, counts);
    return DSA_OK;
}

}  // namespace
}  // namespace dsa

using namespace dsa;

DSA_EXPORT int dsa_vq_search(const void* x, const void* codebook, int64_t T, int64_t K, int64_t L, int32_t dtype, void* indices, void* xq,
                             void* partial, void* total, double scale, void* stream)
{
    const char* route = "";
    if (int rc = vq_check(route, VQ_SEARCH, T, K, L, dtype)) return rc;
    if (T == 0) return DSA_OK;
    if (!(x && codebook && indices && partial)) return fail(DSA_ERR_INVALID_ARGUMENT, "vq: null pointer");
    const int rc = with_dtype(dtype, "vq", [&](auto tag) {
        return vq_search<decltype(tag)>(x, codebook, T, K, L, indices, xq, partial, total, scale, (hipStream_t)stream);
    });
    return rc ? rc : check_launch(route);
}

DSA_EXPORT int64_t dsa_vq_accum_workspace_bytes(int64_t T, int64_t K, int64_t L)
{
    const char* route = "";
    if (vq_check(route, VQ_ACCUM, T, K, L, DSA_F32)) return -1;
    return (int64_t)vq_accum_segments(T, K, L) * K * (L + 1) * 8;
}

DSA_EXPORT int dsa_vq_accum(const void* x, const void* indices, int64_t T, int64_t K, int64_t L, int32_t dtype, void* workspace, void* stream)
{
    const char* route = "";
    if (int rc = vq_check(route, VQ_ACCUM, T, K, L, dtype)) return rc;
    if (T == 0) return DSA_OK;
    if (!(x && indices && workspace)) return fail(DSA_ERR_INVALID_ARGUMENT, "vq: null pointer");
    const int rc = with_dtype(dtype, "vq", [&](auto tag) { return vq_accum<decltype(tag)>(x, indices, T, K, L, workspace, (hipStream_t)stream); });
    return rc ? rc : check_launch(route);
}

DSA_EXPORT int dsa_vq_update(const void* workspace, const void* partial, int64_t n_partial, int64_t T, int64_t K, int64_t L, int64_t min_data,
                             void* n_data, void* pending, void* readback, void* stream)
{
    const char* route = "";
    if (int rc = vq_check(route, VQ_UPDATE, T, K, L, DSA_F32)) return rc;
    if (T == 0) return DSA_OK;
    if (!(workspace && n_data && pending && readback) || (n_partial > 0 && !partial)) return fail(DSA_ERR_INVALID_ARGUMENT, "vq: null pointer");
    if (min_data < 1 || n_partial < 0) return fail(DSA_ERR_INVALID_ARGUMENT, "vq: invalid options");
    const int nseg = vq_accum_segments(T, K, L);
    const double* sums = (const double*)workspace;
    const int64_t* counts = (const int64_t*)(sums + (int64_t)nseg * K * L);
    hipLaunchKernelGGL(vq_update_kernel, dim3((unsigned)K), dim3(256), 0, (hipStream_t)stream, sums, counts, nseg, (int)K, (int)L, (long)min_data,
                       (int64_t*)n_data, (float*)pending);
    hipLaunchKernelGGL(vq_readback_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const int64_t*)n_data, (int)K, (const double*)partial,
                       (long)n_partial, (double)T, (long)min_data, (double*)readback);
    return check_launch(route);
}

DSA_EXPORT int dsa_vq_lookup(const void* indices, const void* codebook, int64_t T, int64_t K, int64_t L, int32_t dtype, void* xq, void* stream)
{
    const char* route = "";
    if (int rc = vq_check(route, VQ_LOOKUP, T, K, L, dtype)) return rc;
    if (T == 0) return DSA_OK;
    if (!(indices && codebook && xq)) return fail(DSA_ERR_INVALID_ARGUMENT, "vq: null pointer");
    const int64_t n = T * L;
    const dim3 grid((unsigned)((n + 255) / 256));
    return with_dtype(dtype, "vq", [&](auto tag) {
        using V = decltype(tag);   // (T is the entry's row count)
        hipLaunchKernelGGL((vq_lookup_kernel<V>), grid, dim3(256), 0, (hipStream_t)stream, (const int64_t*)indices, (const float*)codebook, (long)n,
                           (int)K, (int)L, (V*)xq);
        return check_launch(route);
    });
}

DSA_EXPORT int dsa_vq_vjp(const void* g_xq, const void* g_loss, const void* x, const void* xq, int64_t n, int32_t dtype, void* gx, void* stream)
{
    const char* route = "";
    if (int rc = vq_check(route, VQ_VJP, n, 1, 1, dtype)) return rc;
    if (n == 0) return DSA_OK;
    if (!gx || (g_loss && !(x && xq))) return fail(DSA_ERR_INVALID_ARGUMENT, "vq: null pointer");
    const dim3 grid((unsigned)((n + 255) / 256));
    return with_dtype(dtype, "vq", [&](auto tag) {
        using T = decltype(tag);
        hipLaunchKernelGGL((vq_vjp_kernel<T>), grid, dim3(256), 0, (hipStream_t)stream, (const T*)g_xq, (const T*)g_loss, (const T*)x, (const T*)xq,
                           (long)n, (T*)gx);
        return check_launch(route);
    });
}
