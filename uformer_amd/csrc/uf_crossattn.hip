// Cross-modulator attention of a decoder LeWin block (reference LeWinTransformerBlock.forward with cross_modulator=True, model.py:945-949, through
// Attention.forward :549-595 and LinearProjection.forward with attn_kv :431-442), in place on the f32 token stream:
//
//   x[m] += proj( softmax( (x[m] Wq^T + bq) hd^-0.5 . K_h^T ) V_h )            K | V = to_kv(cross_modulator.weight): 64 learned tokens, the same for every row
//
// There is no LayerNorm (the reference computes norm_cross(x) and discards it), no window geometry, no bias table and no mask: the branch is row-local
// given the 64 shared keys / values, which the caller projects once per parameter version.  One workgroup (4 waves) owns ROWS = 64 consecutive token
// rows (32 for f32 at C = 512, where two 64-row tiles do not fit the LDS):
//   phase 1  the x rows, rounded to T, into the LDS tile Xs[ROWS][C];
//   phase 2  q = (Xs Wq^T + bq) hd^-0.5, rounded to T, into the LDS tile Qs[ROWS][C]: Wq streamed from the fragment-major pack (L2) through a register
//            ring; the output columns (and, below C = 64, the rows) are split over the waves;
//   phase 3  per (head, 16-query tile) unit, one wave: S^T = K_h Q^T (f32), softmax over the 64 keys in f32 (2-byte types: in the log2 domain),
//            e rounded to T as the operand of O^T = V_h^T E^T, o = O / sum(e) rounded to T into Xs (the x tile is dead by then);
//   phase 4  x += Xs Wp^T + bp: f32 accumulators, f32 bias, f32 residual, 16 bytes per lane; the stream is not rounded.
// The operand layouts of phase 3 are those of uf_attn.hip (the P registers of S^T are the B operand of O^T, V is read transposed).
// Every index is bounded by construction: M is a multiple of 64 (no row tail), tile counts are compile-time divisors of C, the ring never
// requests a k-step past the last.
#include <math.h>

#include "uf_internal.h"

namespace uf {
namespace {

struct CrossParams {
    float* x; int ld;
    const void* wq; const float* bq;
    const void* k; const void* vt;
    const void* wp; const float* bp;
    float qscale;
};

constexpr float CROSS_LOG2E = 1.4426950408889634f;

template <typename T> struct PFragX {  // the P operand from exp'ed scores, as uf_attn.hip
    static __device__ __forceinline__ void make(Frag<T>& f, f32x4 a, f32x4 b) {
        f.v = u32x4{pack2<T>(a[0], a[1]), pack2<T>(a[2], a[3]), pack2<T>(b[0], b[1]), pack2<T>(b[2], b[3])};
    }
};
template <> struct PFragX<float> {
    static __device__ __forceinline__ void make(Frag<float>& f, f32x4 a, f32x4 b) { f.lo = a; f.hi = b; }
};
// V^T operand: 4 keys at p0 and 4 keys at p1
template <typename T> __device__ __forceinline__ void load_vtx(Frag<T>& f, const T* p0, const T* p1) {
    static_assert(sizeof(T) == 2, "2-byte operand type");
    const u32x2 a = *reinterpret_cast<const u32x2*>(p0);
    const u32x2 b = *reinterpret_cast<const u32x2*>(p1);
    f.v = u32x4{a[0], a[1], b[0], b[1]};
}
__device__ __forceinline__ void load_vtx(Frag<float>& f, const float* p0, const float* p1) {
    f.lo = *reinterpret_cast<const f32x4*>(p0);
    f.hi = *reinterpret_cast<const f32x4*>(p1);
}

template <typename T, int C> struct CrossCfg {
    static constexpr int SZ = sizeof(T);
    static constexpr int ROWS = (SZ == 4 && C == 512) ? 32 : 64;       // f32 at C = 512: two 64-row tiles are 258 KiB
    static constexpr int SA = C * SZ + 16;                             // LDS row stride (bytes): +16 staggers the banks
    static constexpr int smem = 2 * ROWS * SA;
    static_assert(smem <= 160 * 1024, "LDS budget");
};

template <typename T, int C, int HD>
__global__ __launch_bounds__(256) void cross_attn_kernel(const CrossParams p) {
    using Cfg = CrossCfg<T, C>;
    constexpr int SZ = Cfg::SZ, ROWS = Cfg::ROWS, SA = Cfg::SA;
    constexpr int MT = ROWS / 16;                       // 16-row tiles of the workgroup
    constexpr int KS = (C + 31) / 32;                   // k-steps of both GEMMs
    constexpr int NW_N = (C / 16) < 4 ? (C / 16) : 4;   // waves along the output columns / rows
    constexpr int NW_M = 4 / NW_N;
    constexpr int NT = (C / 16) / NW_N;                 // n-tiles per wave
    constexpr int MTW = MT / NW_M;                      // m-tiles per wave
    constexpr int HEADS = C / HD;
    constexpr int DT = HD / 16;
    static_assert(NT * NW_N * 16 == C && MTW * NW_M == MT && HEADS * HD == C && MTW >= 1, "tiling");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Xs = smem;
    char* Qs = smem + ROWS * SA;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fg = lane >> 4;
    const int m0 = blockIdx.x * ROWS;
    const int wn = wave % NW_N, wm = wave / NW_N;

    Frag<T> wf[2][NT];
    auto wload = [&](const T* w, int ks, int slot) {
#pragma unroll
        for (int i = 0; i < NT; ++i) load_frag(wf[slot][i], w + ((size_t)((wn * NT + i) * KS + ks) * 64 + lane) * 8);
    };
    // acc[i][j] = sum_k W[n-tile i][k] A[m-tile j][k]: a lane holds 4 consecutive output channels of one row per tile
    f32x4 acc[NT][MTW];
    auto gemm = [&](const T* w, const char* As) {
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int j = 0; j < MTW; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        const char* arow = As + (wm * MTW * 16 + fr) * SA + fg * 8 * SZ;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            Frag<T> af[MTW];
#pragma unroll
            for (int j = 0; j < MTW; ++j) {
                if (fg * 8 < C) load_frag(af[j], reinterpret_cast<const T*>(arow + j * 16 * SA + ks * 32 * SZ));
                else af[j].zero();                        // C = 16: k-slots 16..31 are the pack's zero padding
            }
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int j = 0; j < MTW; ++j) mma16(acc[i][j], wf[ks & 1][i], af[j]);
            if (ks + 2 < KS) wload(w, ks + 2, ks & 1);
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    const T* wq = reinterpret_cast<const T*>(p.wq);
    const T* wp = reinterpret_cast<const T*>(p.wp);
    wload(wq, 0, 0);                                      // the first k-steps of Wq travel from L2 while the x tile is staged
    if (KS > 1) wload(wq, 1, 1);

    // ---------------- phase 1: x rows -> T -> Xs ----------------
    {
        constexpr int LPR = C / 4;                        // 16-byte pieces per row
        constexpr int TOT = ROWS * LPR;
#pragma unroll 4
        for (int i = tid; i < TOT; i += 256) {
            const int row = i / LPR, c = (i % LPR) * 4;
            const f32x4 v = *reinterpret_cast<const f32x4*>(p.x + (size_t)(m0 + row) * p.ld + c);
            store4(reinterpret_cast<T*>(Xs + row * SA) + c, v);
        }
    }
    lds_barrier();

    // ---------------- phase 2: q = (Xs Wq^T + bq) hd^-0.5 -> T -> Qs ----------------
    gemm(wq, Xs);
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int n = (wn * NT + i) * 16 + fg * 4;
        const f32x4 bv = *reinterpret_cast<const f32x4*>(p.bq + n);
#pragma unroll
        for (int j = 0; j < MTW; ++j)
            store4(reinterpret_cast<T*>(Qs + ((wm * MTW + j) * 16 + fr) * SA) + n, (acc[i][j] + bv) * p.qscale);
    }
    wload(wp, 0, 0);                                      // Wp's first k-steps travel during the attention phase
    if (KS > 1) wload(wp, 1, 1);
    lds_barrier();                                        // Qs complete; every wave is done reading Xs

    // ---------------- phase 3: per (head, query tile): softmax(q K^T) V -> T -> Xs ----------------
    {
        const T* kk = reinterpret_cast<const T*>(p.k);
        const T* vv = reinterpret_cast<const T*>(p.vt);
#pragma unroll 1
        for (int u = wave; u < HEADS * MT; u += 4) {
            const int h = u / MT, qt = u % MT;
            const T* kp = kk + (size_t)h * 64 * HD;
            const T* vp = vv + (size_t)h * 64 * HD;
            Frag<T> qf, kf[4];
            if (fg * 8 < HD) {
                load_frag(qf, reinterpret_cast<const T*>(Qs + (qt * 16 + fr) * SA) + h * HD + fg * 8);
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) load_frag(kf[kt], kp + (kt * 16 + fr) * HD + fg * 8);
            } else {                                      // head_dim 16: k-slots 16..31 are zero padding
                qf.zero();
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) kf[kt].zero();
            }
            f32x4 s[4];                                   // S^T: query fr, keys 16 kt + 4 fg + r
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) {
                s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
                mma16(s[kt], kf[kt], qf);
            }
            if constexpr (SZ == 2) {
#pragma unroll
                for (int kt = 0; kt < 4; ++kt) s[kt] *= CROSS_LOG2E;
            }
            float mx = -3.0e38f;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[kt][r]);
            mx = red_xor32<RedMax>(red_xor16<RedMax>(mx));
            float sum = 0.f;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float e;
                    if constexpr (SZ == 2) e = __builtin_amdgcn_exp2f(s[kt][r] - mx);
                    else e = __expf(s[kt][r] - mx);
                    s[kt][r] = e;
                    sum += e;
                }
            sum = red_xor32<RedSum>(red_xor16<RedSum>(sum));
            const float inv = 1.0f / sum;
            f32x4 o[DT];
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int sk = 0; sk < 2; ++sk) {              // 32 keys per step
                Frag<T> pf;
                PFragX<T>::make(pf, s[2 * sk], s[2 * sk + 1]);
#pragma unroll
                for (int dt = 0; dt < DT; ++dt) {
                    Frag<T> vf;
                    const T* row = vp + (dt * 16 + fr) * 64 + sk * 32 + fg * 4;
                    load_vtx(vf, row, row + 16);
                    mma16(o[dt], vf, pf);
                }
            }
#pragma unroll
            for (int dt = 0; dt < DT; ++dt)
                store4(reinterpret_cast<T*>(Xs + (qt * 16 + fr) * SA) + h * HD + dt * 16 + fg * 4, o[dt] * inv);
        }
    }
    lds_barrier();

    // ---------------- phase 4: x += Xs Wp^T + bp ----------------
    gemm(wp, Xs);
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int n = (wn * NT + i) * 16 + fg * 4;
        const f32x4 bv = *reinterpret_cast<const f32x4*>(p.bp + n);
#pragma unroll
        for (int j = 0; j < MTW; ++j) {
            float* px = p.x + (size_t)(m0 + (wm * MTW + j) * 16 + fr) * p.ld + n;
            const f32x4 xv = *reinterpret_cast<const f32x4*>(px);
            *reinterpret_cast<f32x4*>(px) = xv + (acc[i][j] + bv);
        }
    }
}

template <typename T, int C, int HD>
int launch_one(const CrossParams& p, int M, hipStream_t st) {
    using Cfg = CrossCfg<T, C>;
    auto kern = cross_attn_kernel<T, C, HD>;
    static bool lds_done[64] = {};
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), Cfg::smem, lds_done, "cross_attn")) return rc;
    char name[96] = "";
    if (timing_enabled()) snprintf(name, sizeof(name), "cross_attn_%s_c%d_hd%d %dx%d", TypeName<T>::s, C, HD, M, C);
    {
        ScopedTimer tm(name, 4.0 * M * C * C + 4.0 * 64.0 * M * C, 8.0 * M * C + (2.0 * C * C + 2.0 * 64 * C) * sizeof(T), st);
        hipLaunchKernelGGL(kern, dim3(M / Cfg::ROWS), dim3(256), Cfg::smem, st, p);
    }
    return check_launch("cross_attn");
}

template <typename T, int C>
int launch_hd(const CrossParams& p, int M, int hd, hipStream_t st) {
    if constexpr (C >= 32) {
        if (hd == 32) return launch_one<T, C, 32>(p, M, st);
    }
    return launch_one<T, C, 16>(p, M, st);
}

template <typename T>
int launch_c(const CrossParams& p, int M, int C, int hd, hipStream_t st) {
    switch (C) {
        case 16: return launch_hd<T, 16>(p, M, hd, st);
        case 32: return launch_hd<T, 32>(p, M, hd, st);
        case 64: return launch_hd<T, 64>(p, M, hd, st);
        case 128: return launch_hd<T, 128>(p, M, hd, st);
        case 256: return launch_hd<T, 256>(p, M, hd, st);
        case 512: return launch_hd<T, 512>(p, M, hd, st);
        default:
            set_error("uf_cross_attn_fwd: C=%d unsupported (16, 32, 64, 128, 256, 512)", C);
            return UF_ERR_UNSUPPORTED;
    }
}

}  // namespace
}  // namespace uf

using namespace uf;

extern "C" int uf_cross_attn_fwd(const uf_cross_params* cp, float* x, int ld, int M, int C, uf_dtype dtype, void* stream) {
    UF_REQUIRE(cp, UF_ERR_NULL, "uf_cross_attn_fwd: p is null");
    UF_REQUIRE(x, UF_ERR_NULL, "uf_cross_attn_fwd: x is null");
    UF_REQUIRE(cp->wq_fm && cp->bq && cp->k && cp->vt && cp->wp_fm && cp->bp, UF_ERR_NULL,
               "uf_cross_attn_fwd: null parameter (wq_fm, bq, k, vt, wp_fm and bp must all be set)");
    UF_REQUIRE(dtype_ok(dtype), UF_ERR_UNSUPPORTED, "uf_cross_attn_fwd: dtype %d", (int)dtype);
    UF_REQUIRE(C == 16 || C == 32 || C == 64 || C == 128 || C == 256 || C == 512, UF_ERR_UNSUPPORTED,
               "uf_cross_attn_fwd: C=%d unsupported (16, 32, 64, 128, 256, 512)", C);
    UF_REQUIRE(cp->heads > 0 && C % cp->heads == 0, UF_ERR_SHAPE, "uf_cross_attn_fwd: heads=%d does not divide C=%d", cp->heads, C);
    const int hd = C / cp->heads;
    UF_REQUIRE(hd == 16 || hd == 32, UF_ERR_UNSUPPORTED, "uf_cross_attn_fwd: heads=%d gives head_dim %d (16 or 32)", cp->heads, hd);
    UF_REQUIRE(M > 0 && M % 64 == 0, UF_ERR_SHAPE, "uf_cross_attn_fwd: M=%d (a positive multiple of 64)", M);
    UF_REQUIRE(ld >= C && ld % 4 == 0, UF_ERR_SHAPE, "uf_cross_attn_fwd: ld=%d (>= C, a multiple of 4)", ld);
    const uintptr_t al = (uintptr_t)x | (uintptr_t)cp->wq_fm | (uintptr_t)cp->bq | (uintptr_t)cp->k | (uintptr_t)cp->vt | (uintptr_t)cp->wp_fm | (uintptr_t)cp->bp;
    UF_REQUIRE((al % 16) == 0, UF_ERR_ALIGN, "uf_cross_attn_fwd: x and the operands of p must be 16-byte aligned");
    UF_REQUIRE((long long)M * ld < 0x7fffffffLL * 4, UF_ERR_SHAPE, "uf_cross_attn_fwd: M * ld too large");
    CrossParams p{};
    p.x = x; p.ld = ld; p.wq = cp->wq_fm; p.bq = cp->bq; p.k = cp->k; p.vt = cp->vt; p.wp = cp->wp_fm; p.bp = cp->bp;
    p.qscale = (float)(1.0 / sqrt((double)hd));          // q = q * scale (model.py:569)
    hipStream_t st = (hipStream_t)stream;
    UF_DISPATCH(dtype, TT, return launch_c<TT>(p, M, C, hd, st));
    return UF_OK;
}
