// Fused feed-forward half of a LeWin block built with token_mlp = 'ffn' / 'mlp' (reference Mlp, model.py:623-642, :987):
//
//   x[m] += scale[image of m] * ( GELU( LN2(x[m]) W1^T + b1 ) W2^T + b2 )            in place on the f32 token stream
//
// Unlike LeFF there is no depthwise convolution between the two Linears, so the whole branch is row-local and the 4C-wide hidden
// activations never leave the CU.  One workgroup (4 waves) owns 64 token rows:
//   phase 0  LayerNorm of the 64 rows, once, into an operand-type LDS tile As[64][C] (as uf_lngemm.hip);
//   per chunk of HC hidden columns (128; 64 at C = 16 and for f32 at C = 512):
//     fc1    wave w computes the chunk's n-tiles {w, w + 4} x all 64 rows: weight fragments streamed from the fragment-major pack
//            (L2) through a register ring, activation fragments from As;
//     act    + b1, gelu_n<T> (the flavour attn_block phase 3 / ln_gemm apply), rounded to T into the LDS tile Hs[64][HC];
//     fc2    acc[64][C] += Hs W2[:, chunk]^T: the C output columns (and, below C = 64, the rows) are split over the waves, the
//            f32 accumulators stay in registers for the whole kernel (C / 4 VGPRs per lane);
//   epilogue x += scale * (acc + b2), 16 bytes per lane.
// Hs is double buffered where LDS allows (one workgroup barrier per chunk), else single buffered with two.
// Every index is bounded by construction: M is a multiple of 64 (no row tail), the chunk / tile counts are compile-time divisors
// of C and 4C, and the weight prefetch past the last chunk is clamped to the last chunk.
#include <type_traits>

#include "uf_internal.h"

namespace uf {
namespace {

struct FfnParams {
    float* x; int ld;
    const float* gamma; const float* beta;
    const void* w1; const float* b1;     // fragment-major T (4C, C), f32 (4C)
    const void* w2; const float* b2;     // fragment-major T (C, 4C), f32 (C)
    const float* scale; int hw;          // per-image factor of the branch (NULL = 1), tokens per image (a multiple of 64)
};

template <typename T, int C> struct FfnCfg {
    static constexpr int SZ = sizeof(T);
    static constexpr int HID = 4 * C;
    static constexpr bool tight = SZ == 4 && C == 512;                 // f32 at C = 512: the operand tile alone is 129 KiB
    static constexpr int HC = (HID < 128 || tight) ? 64 : 128;         // hidden columns per chunk
    static constexpr int SA = C * SZ + 16;                             // LDS row strides (bytes): +16 staggers the banks
    static constexpr int SH = HC * SZ + 16;
    static constexpr int NBUF = (64 * SA + 2 * 64 * SH <= 160 * 1024) ? 2 : 1;
    static constexpr int smem = 64 * SA + NBUF * 64 * SH;
    static_assert(smem <= 160 * 1024, "LDS budget");
};

template <typename T, int C>
__global__ __launch_bounds__(256) void ffn_kernel(const FfnParams p) {
    using Cfg = FfnCfg<T, C>;
    constexpr int SZ = Cfg::SZ, HID = Cfg::HID, HC = Cfg::HC, SA = Cfg::SA, SH = Cfg::SH, NBUF = Cfg::NBUF;
    constexpr int NCH = HID / HC;                    // chunks
    constexpr int NT1 = HC / 64;                     // fc1 n-tiles per wave and chunk
    constexpr int KS1 = (C + 31) / 32;               // fc1 k-steps
    constexpr int R1 = KS1 < 4 ? KS1 : 4;            // fc1 weight ring (k-steps in flight); divides KS1
    constexpr int KSC = HC / 32;                     // fc2 k-steps per chunk
    constexpr int KS2 = HID / 32;                    // k-steps of a whole W2 row tile
    constexpr int NW_N = (C / 16) < 4 ? (C / 16) : 4;   // waves along the output columns / rows of fc2
    constexpr int NW_M = 4 / NW_N;
    constexpr int NT2 = (C / 16) / NW_N;             // fc2 n-tiles per wave
    constexpr int MT2 = 4 / NW_M;                    // fc2 m-tiles per wave
    static_assert(KS1 % R1 == 0 && HID % HC == 0 && NT2 * NW_N * 16 == C && MT2 * NW_M == 4, "tiling");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* As = smem;
    char* Hs = smem + 64 * SA;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fg = lane >> 4;
    const int m0 = blockIdx.x * 64;
    const T* w1 = reinterpret_cast<const T*>(p.w1);
    const T* w2 = reinterpret_cast<const T*>(p.w2);

    // fc1 weight ring: slot s holds k-step (q % KS1) of chunk (q / KS1) for the flat sequence q = s, s + R1, ...
    Frag<T> w1f[R1][NT1];
    auto w1load = [&](int c, int ks, int slot) {
#pragma unroll
        for (int i = 0; i < NT1; ++i)
            load_frag(w1f[slot][i], w1 + ((size_t)((c * (HC / 16) + i * 4 + wave) * KS1 + ks) * 64 + lane) * 8);
    };
#pragma unroll
    for (int s = 0; s < R1; ++s) w1load(0, s, s);

    // ---------------- phase 0: LayerNorm of the 64 rows into As (uf_lngemm.hip phase 0 without gather / modulator) ----------------
    {
        constexpr int LPR = (C / 4) < 64 ? (C / 4) : 64;
        constexpr int V4 = C / (4 * LPR);
        constexpr int RPP = 256 / LPR;
        constexpr int NP = 64 / RPP;
        constexpr int U = (16 / V4) < NP ? (16 / V4) : NP;
        static_assert(NP % U == 0, "pass batching");
        const int sub = tid % LPR;
#pragma unroll 1
        for (int r0 = 0; r0 < 64; r0 += RPP * U) {
            f32x4 v[U][V4];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int m = m0 + r0 + u * RPP + tid / LPR;
#pragma unroll
                for (int i = 0; i < V4; ++i) v[u][i] = *reinterpret_cast<const f32x4*>(p.x + (size_t)m * p.ld + (i * LPR + sub) * 4);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int row = r0 + u * RPP + tid / LPR;
                float sum = 0.f;
#pragma unroll
                for (int i = 0; i < V4; ++i) sum += (v[u][i][0] + v[u][i][1]) + (v[u][i][2] + v[u][i][3]);
                sum = allreduce<RedSum, LPR>(sum);
                const float mean = sum * (1.0f / C);
                float sq = 0.f;
#pragma unroll
                for (int i = 0; i < V4; ++i) {
                    v[u][i] -= mean;
                    sq += (v[u][i][0] * v[u][i][0] + v[u][i][1] * v[u][i][1]) + (v[u][i][2] * v[u][i][2] + v[u][i][3] * v[u][i][3]);
                }
                sq = allreduce<RedSum, LPR>(sq);
                const float rstd = 1.0f / sqrtf(sq * (1.0f / C) + 1e-5f);
#pragma unroll
                for (int i = 0; i < V4; ++i) {
                    const int c = (i * LPR + sub) * 4;
                    const f32x4 y = v[u][i] * rstd * *reinterpret_cast<const f32x4*>(p.gamma + c) + *reinterpret_cast<const f32x4*>(p.beta + c);
                    store4(reinterpret_cast<T*>(As + row * SA) + c, y);
                }
            }
        }
    }
    lds_barrier();

    const int wn = wave % NW_N, wm = wave / NW_N;
    f32x4 acc2[NT2][MT2];
#pragma unroll
    for (int i = 0; i < NT2; ++i)
#pragma unroll
        for (int j = 0; j < MT2; ++j) acc2[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    Frag<T> w2f[2][NT2];
    auto w2load = [&](int c, int kk, int slot) {
#pragma unroll
        for (int i = 0; i < NT2; ++i)
            load_frag(w2f[slot][i], w2 + ((size_t)((wn * NT2 + i) * KS2 + c * KSC + kk) * 64 + lane) * 8);
    };
    const char* arow = As + fr * SA + fg * 8 * SZ;

#pragma unroll 1
    for (int c = 0; c < NCH; ++c) {
        char* Hb = Hs + (NBUF == 2 ? (c & 1) : 0) * (64 * SH);
        const int cn = c + 1 < NCH ? c + 1 : NCH - 1;     // the ring's refill past the last chunk re-reads the last chunk (in bounds, unused)
        // this chunk's first two fc2 k-steps travel from L2 while fc1 runs
        w2load(c, 0, 0);
        w2load(c, 1, 1);
        __builtin_amdgcn_sched_barrier(0);

        // ---- fc1: Hs[64][HC] = As W1[chunk]^T ----
        f32x4 acc1[NT1][4];
#pragma unroll
        for (int i = 0; i < NT1; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc1[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS1; ++ks) {
            Frag<T> af[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (fg * 8 < C) load_frag(af[j], reinterpret_cast<const T*>(arow + j * 16 * SA + ks * 32 * SZ));
                else af[j].zero();                        // C = 16: k-slots 16..31 are the pack's zero padding
            }
#pragma unroll
            for (int i = 0; i < NT1; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) mma16(acc1[i][j], w1f[ks % R1][i], af[j]);
            if (ks + R1 < KS1) w1load(c, ks + R1, ks % R1);
            else w1load(cn, ks + R1 - KS1, ks % R1);
            __builtin_amdgcn_sched_barrier(0);
        }

        // ---- + b1, GELU, round to T: a lane holds 4 consecutive hidden channels of one token per tile ----
#pragma unroll
        for (int i = 0; i < NT1; ++i) {
            const int hc = (i * 4 + wave) * 16 + fg * 4;
            const f32x4 bv = *reinterpret_cast<const f32x4*>(p.b1 + c * HC + hc);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                f32x4 v = acc1[i][j] + bv;
                gelu4<T>(v);
                store4(reinterpret_cast<T*>(Hb + (j * 16 + fr) * SH) + hc, v);
            }
        }
        lds_barrier();

        // ---- fc2: acc2 += Hs W2[:, chunk]^T ----
        const char* hrow = Hb + (wm * MT2 * 16 + fr) * SH + fg * 8 * SZ;
#pragma unroll
        for (int kk = 0; kk < KSC; ++kk) {
            Frag<T> hf[MT2];
#pragma unroll
            for (int j = 0; j < MT2; ++j) load_frag(hf[j], reinterpret_cast<const T*>(hrow + j * 16 * SH + kk * 32 * SZ));
#pragma unroll
            for (int i = 0; i < NT2; ++i)
#pragma unroll
                for (int j = 0; j < MT2; ++j) mma16(acc2[i][j], w2f[kk & 1][i], hf[j]);
            if (kk + 2 < KSC) w2load(c, kk + 2, kk & 1);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (NBUF == 1) lds_barrier();                     // single buffer: every wave is done reading Hs before the next chunk overwrites it
    }

    // ---------------- epilogue: x += scale * (acc + b2) ----------------
    const float s = p.scale ? p.scale[m0 / p.hw] : 1.0f;  // a 64-row tile never straddles two images (hw % 64 == 0)
#pragma unroll
    for (int i = 0; i < NT2; ++i) {
        const int n = (wn * NT2 + i) * 16 + fg * 4;
        const f32x4 bv = *reinterpret_cast<const f32x4*>(p.b2 + n);
#pragma unroll
        for (int j = 0; j < MT2; ++j) {
            float* px = p.x + (size_t)(m0 + (wm * MT2 + j) * 16 + fr) * p.ld + n;
            const f32x4 xv = *reinterpret_cast<const f32x4*>(px);
            *reinterpret_cast<f32x4*>(px) = xv + s * (acc2[i][j] + bv);
        }
    }
}

template <typename T, int C>
int launch_one(const FfnParams& p, int M, hipStream_t st) {
    using Cfg = FfnCfg<T, C>;
    auto kern = ffn_kernel<T, C>;
    static bool lds_done[64] = {};
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), Cfg::smem, lds_done, "ffn")) return rc;
    char name[96] = "";
    if (timing_enabled()) snprintf(name, sizeof(name), "ffn_%s_c%d %dx%d", TypeName<T>::s, C, M, C);
    {
        ScopedTimer tm(name, 16.0 * M * C * C, 8.0 * M * C + 8.0 * C * C * sizeof(T), st);
        hipLaunchKernelGGL(kern, dim3(M / 64), dim3(256), Cfg::smem, st, p);
    }
    return check_launch("ffn");
}

template <typename T>
int launch_c(const FfnParams& p, int M, int C, hipStream_t st) {
    switch (C) {
        case 16: return launch_one<T, 16>(p, M, st);
        case 32: return launch_one<T, 32>(p, M, st);
        case 64: return launch_one<T, 64>(p, M, st);
        case 128: return launch_one<T, 128>(p, M, st);
        case 256: return launch_one<T, 256>(p, M, st);
        case 512: return launch_one<T, 512>(p, M, st);
        default:
            set_error("uf_ffn_fwd: C=%d unsupported (16, 32, 64, 128, 256, 512)", C);
            return UF_ERR_UNSUPPORTED;
    }
}

}  // namespace
}  // namespace uf

using namespace uf;

extern "C" int uf_ffn_fwd(float* x, int ld, const float* gamma, const float* beta, const void* w1_fm, const float* b1, const void* w2_fm,
                          const float* b2, const float* scale, int B, int M, int C, uf_dtype dtype, void* stream) {
    UF_REQUIRE(x && gamma && beta && w1_fm && b1 && w2_fm && b2, UF_ERR_NULL, "uf_ffn_fwd: null pointer");
    UF_REQUIRE(dtype_ok(dtype), UF_ERR_UNSUPPORTED, "uf_ffn_fwd: dtype %d", (int)dtype);
    UF_REQUIRE(C == 16 || C == 32 || C == 64 || C == 128 || C == 256 || C == 512, UF_ERR_UNSUPPORTED,
               "uf_ffn_fwd: C=%d unsupported (16, 32, 64, 128, 256, 512)", C);
    UF_REQUIRE(B > 0 && M > 0 && M % 64 == 0 && M % B == 0 && (M / B) % 64 == 0, UF_ERR_SHAPE,
               "uf_ffn_fwd: M=%d B=%d (M and the tokens per image M / B must be multiples of 64)", M, B);
    UF_REQUIRE(ld >= C && ld % 4 == 0, UF_ERR_ALIGN, "uf_ffn_fwd: ld=%d (>= C, a multiple of 4)", ld);
    const uintptr_t al = (uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)w1_fm | (uintptr_t)b1 | (uintptr_t)w2_fm | (uintptr_t)b2;
    UF_REQUIRE((al % 16) == 0, UF_ERR_ALIGN, "uf_ffn_fwd: operands must be 16-byte aligned");
    UF_REQUIRE((long long)M * ld < 0x7fffffffLL * 4, UF_ERR_SHAPE, "uf_ffn_fwd: tensor too large");
    FfnParams p{};
    p.x = x; p.ld = ld; p.gamma = gamma; p.beta = beta; p.w1 = w1_fm; p.b1 = b1; p.w2 = w2_fm; p.b2 = b2; p.scale = scale; p.hw = M / B;
    hipStream_t st = (hipStream_t)stream;
    UF_DISPATCH(dtype, TT, return launch_c<TT>(p, M, C, st));
    return UF_OK;
}
