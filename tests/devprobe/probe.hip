// TEST-ONLY probe library (tests/devprobe_util.py builds it, tests/test_devprobe_*.py use it): small kernels that include the hot path's
// helper headers AS THEY ARE -- csrc/mht_wave.h, csrc/mht_uf.h, csrc/mht_vtab.h -- and call one helper each, so that a test can say
// which primitive broke.  Not part of pymht_amd.build.SOURCES, nothing of libmht_amd.so or its ABI depends on it.
// Every launcher takes device pointers, launches on the NULL stream, synchronises and returns the hipError_t as an int (-1: refused
// arguments).  No kernel here waits for another thread; the only loops with a wait in them are the headers' own, which carry their bound.
#include "mht_wave.h"
#include "mht_uf.h"
#include "mht_vtab.h"

using namespace mht;
typedef unsigned long long u64;

namespace {

int finish() {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    return (int)hipDeviceSynchronize();
}
// the wavefront helpers want every lane active: whole wavefronts in blocks of 64 or 256 threads only
bool wave_shape(int block, int n) { return (block == 64 || block == 256) && n > 0 && n % block == 0; }

// ---- mht_wave.h: wavefront w works on elements [64 w, 64 w + 64), every lane writes its result --------------------------------------
__global__ void k_scan_u32(const unsigned* in, unsigned* out) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    out[g] = wave_scan_u32(in[g]);
}
// the grow launch's two-half idiom (mht_fgrow_dev.h: child counts of a chunk of up to 128 leaves): wavefront w works on 128 elements
__global__ void k_scan_halves(const unsigned* in, unsigned* out) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x, w = g >> 6, lane = g & 63;
    const int m0 = (int)in[(size_t)w * 128 + lane], m1 = (int)in[(size_t)w * 128 + 64 + lane];
    const int i0 = (int)wave_scan_u32((unsigned)m0);
    const int i1 = (int)wave_scan_u32((unsigned)m1) + __builtin_amdgcn_readlane(i0, 63);
    out[(size_t)w * 128 + lane] = (unsigned)i0;
    out[(size_t)w * 128 + 64 + lane] = (unsigned)i1;
}
__global__ void k_sum_i32(const int* in, int* out) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    out[g] = wave_sum_i32(in[g]);
}
__global__ void k_min_i32(const int* in, int* out) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    out[g] = wave_min_i32(in[g]);
}
__global__ void k_max_i32(const int* in, int* out) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    out[g] = wave_max_i32(in[g]);
}
// the four-value bounding-box reduction of the grow launch, back to back: in / out are [4][n]
__global__ void k_box_i32(const int* in, int* out, int n) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    int b0 = in[g], b1 = in[(size_t)n + g], b2 = in[2 * (size_t)n + g], b3 = in[3 * (size_t)n + g];
    b0 = wave_min_i32(b0); b1 = wave_max_i32(b1); b2 = wave_min_i32(b2); b3 = wave_max_i32(b3);
    out[g] = b0; out[(size_t)n + g] = b1; out[2 * (size_t)n + g] = b2; out[3 * (size_t)n + g] = b3;
}
__global__ void k_sum_f64(const double* in, double* out) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    out[g] = wave_sum(in[g]);
}
__global__ void k_min_value(const double* in, double* out) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    out[g] = wave_min_value(in[g]);
}
__global__ void k_row16_min_value(const double* in, double* out) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    out[g] = row16_min_value(in[g]);
}
__global__ void k_min_pair(const double* vin, const int* iin, double* vout, int* iout) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    double v = vin[g];
    int i = iin[g];
    wave_min_pair(v, i);
    vout[g] = v; iout[g] = i;
}
__global__ void k_row16_min_pair(const double* vin, const int* iin, double* vout, int* iout) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    double v = vin[g];
    int i = iin[g];
    row16_min_pair(v, i);
    vout[g] = v; iout[g] = i;
}

// ---- mht_uf.h ----------------------------------------------------------------------------------------------------------------------
// one edge per thread
__global__ void k_uf_link(u64* parent, int T, unsigned epoch, const int* ex, const int* ey, int E) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E) return;
    const int x = ex[g], y = ey[g];
    if (x >= 0 && x < T && y >= 0 && y < T) uf_link(parent, epoch, x, y);      // (an edge outside the table is dropped: the test sees it missing)
}
// shaped like the grow launch's target workgroup: one workgroup of 256 per target, its association bitset (AW words) goes to LDS, the
// LAST wavefront exchanges the owner words (uf_claim, conflict list of `cap` entries in LDS) and, behind a barrier, links the list
__global__ __launch_bounds__(256) void k_uf_claim(const u64* assoc, int AW, u64* owner, u64* parent, unsigned epoch, int cap, int* nconf_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u64* tb = reinterpret_cast<u64*>(smem);
    int* conf = reinterpret_cast<int*>(tb + AW);
    __shared__ int s_nconf;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, pos = blockIdx.x;
    for (int w = tid; w < AW; w += blockDim.x) tb[w] = assoc[(size_t)pos * AW + w];
    if (tid == 0) s_nconf = -1;
    __syncthreads();
    if (wave == 3) uf_claim(owner, parent, epoch, pos, tb, AW, lane, conf, cap, &s_nconf);
    __syncthreads();
    if (wave == 3) {
        for (int i = lane; i < s_nconf; i += 64) uf_link(parent, epoch, pos, conf[i]);
        if (lane == 0) nconf_out[pos] = s_nconf;
    }
}

// ---- mht_vtab.h ----------------------------------------------------------------------------------------------------------------------
// one request per thread: req[g] names a value of the list (kind 0: float32 covariance, words = its NP floats; kind 1: float64, words =
// its NP doubles; kind 2: promotion of the float32 value whose id is words[0]); ids[g] = what the table answered
__global__ void k_vt_insert(const VTab t, int n, const int* req, int n_values, const int* kind, const u64* words, const double* pd, int* ids) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const int v = req[g];
    if (v < 0 || v >= n_values) { ids[g] = -1; return; }
    const u64* w = words + (size_t)v * (2 * VT_PW);
    if (kind[v] == 0) {
        float P[NP];
#pragma unroll
        for (int q = 0; q < VT_PW; ++q) { P[2 * q] = __uint_as_float((unsigned)w[q]); P[2 * q + 1] = __uint_as_float((unsigned)(w[q] >> 32)); }
        ids[g] = vt_find_or_insert(t, P, pd[v]);
    } else if (kind[v] == 1) {
        double P[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) P[q] = __longlong_as_double((long long)w[q]);
        ids[g] = vt_find_or_insert64(t, P, pd[v]);
    } else {
        double P64[NP];
        const int id32 = (int)w[0];
        ids[g] = (id32 >= 0 && id32 < t.vcap) ? vt_promote(t, id32, pd[v], P64) : -1;
    }
}
// vt_load / vt_load64 of an id per thread: out[g] = 2 * VT_PW words (a float32 value fills the first VT_PW)
__global__ void k_vt_load(const VTab t, int n, const int* ids, const int* kind, u64* out) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    u64* o = out + (size_t)g * (2 * VT_PW);
    if (ids[g] < 0 || ids[g] + (kind[g] ? 1 : 0) >= t.vcap) {      // (not an id of this table: the test sees zeros)
        for (int q = 0; q < 2 * VT_PW; ++q) o[q] = 0ull;
        return;
    }
    if (kind[g] == 0) {
        float P[NP];
        vt_load(t, ids[g], P);
#pragma unroll
        for (int q = 0; q < VT_PW; ++q) o[q] = ((u64)__float_as_uint(P[2 * q + 1]) << 32) | __float_as_uint(P[2 * q]);
    } else {
        double P[NP];
        vt_load64(t, ids[g], P);
#pragma unroll
        for (int q = 0; q < NP; ++q) o[q] = (u64)__double_as_longlong(P[q]);
    }
}

}  // namespace

extern "C" {

// the constants of this build that the tests size their arrays by: {NX, NP, VT_PW, GKQ}
int probe_constants(int* out) { out[0] = NX; out[1] = NP; out[2] = VT_PW; out[3] = GKQ; return 0; }

#define WAVE_PROBE_1(name, kernel, T)                                   \
    int name(int block, int n, const T* in, T* out) {                   \
        if (!wave_shape(block, n)) return -1;                           \
        hipLaunchKernelGGL(kernel, dim3(n / block), dim3(block), 0, nullptr, in, out); \
        return finish();                                                \
    }
WAVE_PROBE_1(probe_scan_u32, k_scan_u32, unsigned)
WAVE_PROBE_1(probe_sum_i32, k_sum_i32, int)
WAVE_PROBE_1(probe_min_i32, k_min_i32, int)
WAVE_PROBE_1(probe_max_i32, k_max_i32, int)
WAVE_PROBE_1(probe_sum_f64, k_sum_f64, double)
WAVE_PROBE_1(probe_min_value, k_min_value, double)
WAVE_PROBE_1(probe_row16_min_value, k_row16_min_value, double)
#undef WAVE_PROBE_1

// n = threads; in / out hold 2 n elements
int probe_scan_halves(int block, int n, const unsigned* in, unsigned* out) {
    if (!wave_shape(block, n)) return -1;
    hipLaunchKernelGGL(k_scan_halves, dim3(n / block), dim3(block), 0, nullptr, in, out);
    return finish();
}
// in / out hold 4 n elements
int probe_box_i32(int block, int n, const int* in, int* out) {
    if (!wave_shape(block, n)) return -1;
    hipLaunchKernelGGL(k_box_i32, dim3(n / block), dim3(block), 0, nullptr, in, out, n);
    return finish();
}
int probe_min_pair(int block, int n, const double* vin, const int* iin, double* vout, int* iout) {
    if (!wave_shape(block, n)) return -1;
    hipLaunchKernelGGL(k_min_pair, dim3(n / block), dim3(block), 0, nullptr, vin, iin, vout, iout);
    return finish();
}
int probe_row16_min_pair(int block, int n, const double* vin, const int* iin, double* vout, int* iout) {
    if (!wave_shape(block, n)) return -1;
    hipLaunchKernelGGL(k_row16_min_pair, dim3(n / block), dim3(block), 0, nullptr, vin, iin, vout, iout);
    return finish();
}

// parent: T words
int probe_uf_link(u64* parent, int T, unsigned epoch, const int* ex, const int* ey, int E) {
    if (E < 0 || T <= 0) return -1;
    if (E == 0) return finish();
    hipLaunchKernelGGL(k_uf_link, dim3((E + 255) / 256), dim3(256), 0, nullptr, parent, T, epoch, ex, ey, E);
    return finish();
}
// assoc: [T][AW] words, owner: AW * 64 words, parent: T words, nconf_out: T ints
int probe_uf_claim(const u64* assoc, int T, int AW, u64* owner, u64* parent, unsigned epoch, int cap, int* nconf_out) {
    if (T <= 0 || AW <= 0 || cap < 0) return -1;
    const size_t lds = (size_t)AW * 8 + (size_t)cap * 4;
    if (lds > 32 * 1024) return -1;
    hipLaunchKernelGGL(k_uf_claim, dim3(T), dim3(256), lds, nullptr, assoc, AW, owner, parent, epoch, cap, nconf_out);
    return finish();
}

static VTab make_vtab(u64* Pv, double* pdv, void* Gk, int32_t* child, u64* slots, unsigned* count, int32_t* overflow, int vcap, unsigned hmask) {
    VTab t;
    t.Pv = Pv; t.pdv = pdv; t.Gk = static_cast<float4*>(Gk); t.child = child; t.slots = slots; t.count = count; t.overflow = overflow;
    t.vcap = vcap; t.hmask = hmask;
    return t;
}
// the table: Pv [vcap][VT_PW] words, pdv [vcap], Gk [2 vcap][GKQ] float4, child [2 vcap], slots [hmask + 1], count, overflow.
// requests: req [n] -> kind / words [n_values][2 VT_PW] / pd by value
int probe_vt_insert(u64* Pv, double* pdv, void* Gk, int32_t* child, u64* slots, unsigned* count, int32_t* overflow, int vcap, unsigned hmask,
                    int n, const int* req, int n_values, const int* kind, const u64* words, const double* pd, int* ids) {
    if (n <= 0 || n_values <= 0 || vcap <= 0 || (hmask & (hmask + 1u)) != 0u) return -1;
    hipLaunchKernelGGL(k_vt_insert, dim3((n + 255) / 256), dim3(256), 0, nullptr, make_vtab(Pv, pdv, Gk, child, slots, count, overflow, vcap, hmask), n, req,
                       n_values, kind, words, pd, ids);
    return finish();
}
int probe_vt_load(u64* Pv, double* pdv, void* Gk, int32_t* child, u64* slots, unsigned* count, int32_t* overflow, int vcap, unsigned hmask,
                  int n, const int* ids, const int* kind, u64* out) {
    if (n <= 0 || vcap <= 0) return -1;
    hipLaunchKernelGGL(k_vt_load, dim3((n + 255) / 256), dim3(256), 0, nullptr, make_vtab(Pv, pdv, Gk, child, slots, count, overflow, vcap, hmask), n, ids, kind,
                       out);
    return finish();
}

}  // extern "C"
