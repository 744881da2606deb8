// LayerNorm-fused, A-stationary GEMM for the two K = C projections of a LeWin block:
//
//   LN1 -> roll -> window_partition -> (+modulator) -> [to_q | to_kv]      (model.py:952-969, :431-442)
//   LN2 -> linear1 -> GELU                                                  (model.py:987, :657-658)
//
// One workgroup owns BM token rows.  Phase 0 reads those rows of the f32 residual stream ONCE
// (gathered through the roll/partition index for the norm1 path), normalises them in registers
// and leaves the bf16/f32 operand tile [BM][C] in LDS -- the normalised activations never touch
// HBM.  Phase 1 has no barriers: the four waves walk over 64x64 output units; a wave streams the
// weight fragments of its unit straight from L2 into registers (3-deep software ring, each
// weight row is read by exactly one wave of the block), reads activation fragments from LDS and
// issues 16 MFMAs per k-step.  The epilogue stages 16 rows at a time in a private LDS slab and
// writes whole 128/256-byte row segments (q, k, v^T in the attention layout, or the LeFF hidden).
//
// ln_convqkv_kernel (below, uf_ln_convqkv_fwd) is the same producer for a ConvProjection block (token_projection 'conv', model.py:381-410):
// one window per workgroup, and between phase 0 and the unit walk of each third of the 3C columns a depthwise 3x3 + bias + ReLU over the
// window's own tile, into a second LDS tile.
#include <stdlib.h>

#include <type_traits>

#include "uf_internal.h"

namespace uf {
unsigned long long* debug_get_tbuf();
int launch_layernorm(const float* x, int ld_x, const float* gamma, const float* beta, const float* modulator, void* out,
                     int rows, int H, int W, int C, int windowed, int shift, uf_dtype dtype, hipStream_t st);
namespace {

struct LnGemmParams {
    const float* x; int ld;          // residual stream rows (f32)
    const float* gamma; const float* beta; const float* modulator;
    const void* Wt; const float* bias;  // T[N][C], f32[N]
    int M, N;
    int H, W, windowed, shift;
    void* out; int ldo;              // EP_GELU: T[M][ldo]
    void* q; void* k; void* vt; int heads, hd; float qscale;  // EP_QKV
    unsigned long long* tbuf;        // diagnostic build (UF_STAMPS): cycle stamps (uf_debug_set_tbuf); never read otherwise
};

enum { EP_QKV = 0, EP_GELU = 1 };

template <typename T, int C, int BM, int EP>
__global__ __launch_bounds__(256, 2) void ln_gemm_kernel(const LnGemmParams p) {
    constexpr int SZ = sizeof(T);
    constexpr int EPC = 16 / SZ;
    constexpr int SA = C * SZ + 16;               // LDS row stride of the operand tile
    constexpr int SS = 64 * SZ + 16;              // LDS row stride of a staging slab (16 rows x 64 values)
    constexpr int KS = (C + 31) / 32;             // MFMA k-steps
    constexpr int MH = BM / 64;                   // 64-row halves per block
    constexpr int RING = 3;                       // weight-fragment prefetch depth (k-steps)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* As = smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // provably wave-uniform -> scalar branches / addresses
    const int fr = lane & 15, fg = lane >> 4;
    char* stg = smem + BM * SA + wave * (16 * SS);
    const int m0 = blockIdx.x * BM;
    Census census; census.begin();
    LapTimer<3> ts; ts.start();      // diagnostic build: cycles in the LayerNorm (0), the k-loops (1) and the epilogues (2)

    // ---------------- phase 0: LayerNorm (+gather, +modulator) into LDS -------------------------
    {
        constexpr int LPR = (C / 4) < 64 ? (C / 4) : 64;
        constexpr int V4 = C / (4 * LPR);
        constexpr int RPP = 256 / LPR;                 // rows normalised per pass of the block
        constexpr int NP = BM / RPP;                   // passes
        constexpr int U = (16 / V4) < NP ? (16 / V4) : NP;  // row groups kept in flight (16 x 16-byte loads per thread issued together)
        static_assert(NP % U == 0, "pass batching");
        const int sub = tid % LPR;
#pragma unroll 1
        for (int r0 = 0; r0 < BM; r0 += RPP * U) {
            f32x4 v[U][V4];
            bool live[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int m = m0 + r0 + u * RPP + tid / LPR;
                live[u] = m < p.M;
                const int mc = live[u] ? m : p.M - 1;   // clamped: the load itself is unconditional
                const int src = p.windowed ? window_row_to_token(mc, p.H, p.W, p.shift) : mc;
#pragma unroll
                for (int i = 0; i < V4; ++i) v[u][i] = *reinterpret_cast<const f32x4*>(p.x + (size_t)src * p.ld + (i * LPR + sub) * 4);
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
                    f32x4 y = v[u][i] * rstd * *reinterpret_cast<const f32x4*>(p.gamma + c) + *reinterpret_cast<const f32x4*>(p.beta + c);
                    if (p.modulator) y += *reinterpret_cast<const f32x4*>(p.modulator + (size_t)((m0 + row) & 63) * C + c);  // uniform branch
                    if (!live[u]) y = f32x4{0.f, 0.f, 0.f, 0.f};
                    store4(reinterpret_cast<T*>(As + row * SA) + c, y);
                }
            }
        }
    }
    lds_barrier();
    ts.lap(0);

    // ---------------- phase 1: barrier-free walk over 64 x 64 output units -------------------------
    // blockIdx.y splits the 64-wide column groups when M alone gives too few blocks for 256 CUs
    const int n_groups_all = (p.N + 63) >> 6;
    const int g0 = (int)((long long)n_groups_all * blockIdx.y / gridDim.y);
    const int g1 = (int)((long long)n_groups_all * (blockIdx.y + 1) / gridDim.y);
    const int n_units = MH * (g1 - g0);
    const T* Wt = reinterpret_cast<const T*>(p.Wt);
    const int Cq = p.heads * p.hd;  // == C for the QKV projection
    // Weight loads are UNCONDITIONAL (hipcc wraps a guarded load in an exec-masked branch with a
    // vmcnt(0) wait, which would serialise the prefetch ring): tiles past N are clamped to a valid
    // tile -- their products land in accumulator columns that are never stored.  For C = 16 the packed
    // k-slots 16..31 are zero padding.
    // weights are FRAGMENT-MAJOR (uf_pack_weight_fm): [n-tile][k-step][lane][8] -> one wave-level load
    // reads 1 KiB (bf16) contiguous instead of 16 half cache lines at a power-of-two stride
    const T* wrow[4];
    Frag<T> wf[RING][4];
    auto wload = [&](int ks, int slot) {
#pragma unroll
        for (int i = 0; i < 4; ++i) load_frag(wf[slot][i], wrow[i] + ks * 512);
    };
    // first RING-1 k-steps of a unit's weights; issued for unit u+4 BEFORE the epilogue of unit u so
    // the L2 round trip hides under the epilogue instead of stalling the next unit's first MFMAs.
    auto unit_prefetch = [&](int u) {
        const int nb = (g0 + u / MH) * 64;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int tile = (nb >> 4) + i;                       // clamp: tiles past N are computed but never stored
            tile = tile < (p.N >> 4) ? tile : (p.N >> 4) - 1;
            wrow[i] = Wt + ((size_t)tile * KS * 64 + lane) * 8;
        }
#pragma unroll
        for (int s = 0; s < RING - 1; ++s)
            if (s < KS) wload(s, s);
    };
    if (wave < n_units) unit_prefetch(wave);
#pragma unroll 1
    for (int u = wave; u < n_units; u += 4) {
        ts.lap(2);   // time since the previous k-loop ended = epilogue
        const int mh = u % MH, ng = g0 + u / MH;
        const int nbase = ng * 64, mbase = mh * 64;
        // number of leading n-tiles of this unit that are NOT in the V third (wave-uniform)
        int nv = 4;
        if (EP == EP_QKV) { nv = (2 * Cq - nbase) / 16; nv = nv < 0 ? 0 : (nv > 4 ? 4 : nv); }

        f32x4 acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

        // Software pipeline, pinned with sched_barrier (left alone, hipcc sinks the prefetch loads next
        // to their uses -> vmcnt(1) before every MFMA group -> one L2 round trip per k-step):
        //   weights for k-step ks+2 and activation fragments for ks+1 are issued BEFORE the 16 MFMAs of ks.
        const char* arow = As + (mbase + fr) * SA + fg * 8 * SZ;
        Frag<T> af[2][4];
        auto aload = [&](int ks, int slot) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (fg * 8 < C) load_frag(af[slot][j], reinterpret_cast<const T*>(arow + j * 16 * SA + ks * 32 * SZ));
                else af[slot][j].zero();
            }
        };
        aload(0, 0);
        auto kloop = [&](auto mode_tag) {
            constexpr int MODE = decltype(mode_tag)::value;   // 0: plain tiles, 1: all V tiles, 2: mixed unit
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                if (ks + RING - 1 < KS) wload(ks + RING - 1, (ks + RING - 1) % RING);
                if (ks + 1 < KS) aload(ks + 1, (ks + 1) & 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    // V tiles are computed transposed (lane = channel, 4 consecutive tokens)
                    const bool vt_ = MODE == 1 || (MODE == 2 && i >= nv);
                    if (vt_) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) mma16(acc[i][j], af[ks & 1][j], wf[ks % RING][i]);
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) mma16(acc[i][j], wf[ks % RING][i], af[ks & 1][j]);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        if (EP != EP_QKV || nv == 4) kloop(std::integral_constant<int, 0>{});
        else if (nv == 0) kloop(std::integral_constant<int, 1>{});
        else kloop(std::integral_constant<int, 2>{});
        if (u + 4 < n_units) unit_prefetch(u + 4);
        __builtin_amdgcn_sched_barrier(0);
        ts.lap(1);

        // per-tile destination info for the q/k/v^T layouts, once per unit (scalar): tile i covers
        // channels [nbase+16i, +16) = 16 consecutive d of ONE head of q, k or v.
        int t_h[4], t_d[4], t_w[4];
        if constexpr (EP == EP_QKV) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int nt_ = nbase + i * 16;
                t_w[i] = nt_ / Cq;
                const int c_ = nt_ - t_w[i] * Cq;
                t_h[i] = c_ / p.hd;
                t_d[i] = c_ - t_h[i] * p.hd;
            }
        }

        // ---- epilogue for the LeFF hidden (bf16): no LDS round trip.  A lane holds 4 consecutive channels
        // (8 bytes) of one token per 16-column tile; v_permlane16_swap between lane groups fg and fg^1 of a
        // tile pair turns that into 16 contiguous bytes per lane (guide T21), so one store instruction
        // writes 64 contiguous bytes per token.
        if constexpr (EP == EP_GELU && sizeof(T) == 2) {
            f32x4 bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int n = nbase + i * 16 + fg * 4;
                bv[i] = *reinterpret_cast<const f32x4*>(p.bias + (n < p.N ? n : p.N - 4));
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int m = m0 + mbase + j * 16 + fr;
#pragma unroll
                for (int ip = 0; ip < 4; ip += 2) {              // tile pair (ip, ip+1)
                    f32x4 va = acc[ip][j] + bv[ip], vb = acc[ip + 1][j] + bv[ip + 1];
                    gelu4<T>(va); gelu4<T>(vb);
                    const unsigned a0 = pack2<T>(va[0], va[1]), a1 = pack2<T>(va[2], va[3]);
                    const unsigned b0 = pack2<T>(vb[0], vb[1]), b1 = pack2<T>(vb[2], vb[3]);
                    // after the swap: even fg lanes hold 8 channels of tile ip, odd fg lanes 8 channels of tile ip+1
                    const u32x2_t s0 = __builtin_amdgcn_permlane16_swap(a0, b0, false, false);
                    const u32x2_t s1 = __builtin_amdgcn_permlane16_swap(a1, b1, false, false);
                    const int n = nbase + (ip + (fg & 1)) * 16 + (fg >> 1) * 8;
                    if (m < p.M && n < p.N)
                        *reinterpret_cast<u32x4*>(reinterpret_cast<T*>(p.out) + (size_t)m * p.ldo + n) = u32x4{s0[0], s1[0], s0[1], s1[1]};   // (nontemporal stores measured 3-10 % slower)
                }
            }
        } else
        // ---- epilogue A: [token][channel] tiles (q, k, f32 LeFF hidden): one 16-row m-tile per pass via LDS ----
        if (nv > 0) {
            f32x4 bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int n = nbase + i * 16 + fg * 4;
                bv[i] = *reinterpret_cast<const f32x4*>(p.bias + (n < p.N ? n : p.N - 4));  // clamped, unconditional
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (i < nv) {
                        f32x4 v = acc[i][j] + bv[i];
                        if constexpr (EP == EP_GELU) {
                            gelu4<T>(v);
                        } else {
                            if (nbase + i * 16 < Cq) v *= p.qscale;  // q = q * scale (model.py:497)
                        }
                        store4(reinterpret_cast<T*>(stg + fr * SS) + i * 16 + fg * 4, v);
                    }
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                constexpr int CPR = 64 * SZ / 16;         // 16-byte chunks per staged row
                constexpr int ITERS = 16 * CPR / 64;
#pragma unroll
                for (int it = 0; it < ITERS; ++it) {
                    const int idx = it * 64 + lane;
                    const int r = idx / CPR, cb = idx % CPR;
                    const int m = m0 + mbase + j * 16 + r, n = nbase + cb * EPC;
                    if (m < p.M && n < p.N && (cb * EPC) / 16 < nv) {
                        const u32x4 val = *reinterpret_cast<const u32x4*>(stg + r * SS + cb * 16);
                        T* dst;
                        if constexpr (EP == EP_QKV) {
                            const int ti = (cb * EPC) >> 4;   // 16-column tile of this chunk (lane-constant per pass)
                            const int h = ti == 0 ? t_h[0] : (ti == 1 ? t_h[1] : (ti == 2 ? t_h[2] : t_h[3]));
                            const int d = (ti == 0 ? t_d[0] : (ti == 1 ? t_d[1] : (ti == 2 ? t_d[2] : t_d[3]))) + ((cb * EPC) & 15);
                            const int w = ti == 0 ? t_w[0] : (ti == 1 ? t_w[1] : (ti == 2 ? t_w[2] : t_w[3]));
                            dst = reinterpret_cast<T*>(w == 0 ? p.q : p.k) + (((size_t)(m >> 6) * p.heads + h) * 64 + (m & 63)) * p.hd + d;
                        } else {
                            dst = reinterpret_cast<T*>(p.out) + (size_t)m * p.ldo + n;
                        }
                        *reinterpret_cast<u32x4*>(dst) = val;
                    }
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
        }
        // ---- epilogue B: V^T tiles [channel][token]: one 16-channel n-tile per pass ---------------------
        if (EP == EP_QKV && nv < 4) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (i >= nv) {
                    const int nn = nbase + i * 16 + fr;
                    const float b = p.bias[nn < p.N ? nn : p.N - 1];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const f32x4 v = {acc[i][j][0] + b, acc[i][j][1] + b, acc[i][j][2] + b, acc[i][j][3] + b};
                        store4(reinterpret_cast<T*>(stg + fr * SS) + j * 16 + fg * 4, v);
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    constexpr int CPR = 64 * SZ / 16;
                    constexpr int ITERS = 16 * CPR / 64;
#pragma unroll
                    for (int it = 0; it < ITERS; ++it) {
                        const int idx = it * 64 + lane;
                        const int r = idx / CPR, cb = idx % CPR;
                        const int n = nbase + i * 16 + r, m = m0 + mbase + cb * EPC;
                        if (m < p.M && n < p.N) {
                            const u32x4 val = *reinterpret_cast<const u32x4*>(stg + r * SS + cb * 16);
                            const int h = t_h[i], d = t_d[i] + r;   // tile i of the unit, channel row r
                            T* dst = reinterpret_cast<T*>(p.vt) + (((size_t)(m >> 6) * p.heads + h) * p.hd + d) * 64 + (m & 63);
                            *reinterpret_cast<u32x4*>(dst) = val;
                        }
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                }
            }
        }
    }
    ts.lap(2);
    census.end(p.tbuf, blockIdx.y * gridDim.x + blockIdx.x);
    if constexpr (UF_STAMPS != 0) {
        if (p.tbuf && lane == 0 && (blockIdx.x & 63) == 0 && blockIdx.y == 0) {
            unsigned long long* o = p.tbuf + ((blockIdx.x >> 6) * 4 + wave) * 4;
            o[0] = ts.total(0); o[1] = ts.total(1); o[2] = ts.total(2); o[3] = n_units;
        }
    }
}

template <typename T, int C, int BM, int EP>
int launch_one(const LnGemmParams& p_in, hipStream_t st) {
    constexpr int SZ = sizeof(T);
    constexpr int smem = BM * (C * SZ + 16) + 4 * 16 * (64 * SZ + 16);
    static_assert(smem <= 160 * 1024, "LDS budget");
    auto kern = ln_gemm_kernel<T, C, BM, EP>;
    LnGemmParams p = p_in;
    p.tbuf = debug_get_tbuf();
    static bool lds_done[64] = {};
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), smem, lds_done, "ln_gemm")) return rc;
    char name[96] = "";
    if (timing_enabled())
        snprintf(name, sizeof(name), "ln_gemm_%s_%s_c%d_bm%d %dx%dx%d", TypeName<T>::s, EP == EP_QKV ? "qkv" : "fc1", C, BM, p.M, p.N, C);
    const double mn = (double)p.M * p.N;
    {
        ScopedTimer tm(name, 2.0 * mn * C, (double)p.M * C * 4 + (double)p.N * C * SZ + mn * SZ, st);
        const int mb = (p.M + BM - 1) / BM, groups = (p.N + 63) / 64;
        int nsplit = 1;
        while (mb * nsplit < 512 && nsplit * 2 <= groups) nsplit *= 2;   // >= 2 blocks per CU when possible
        hipLaunchKernelGGL(kern, dim3(mb, nsplit), dim3(256), smem, st, p);
    }
    return check_launch("ln_gemm");
}

template <typename T, int C, int EP>
int launch_bm(const LnGemmParams& p, hipStream_t st) {
    // 128-row blocks when the operand tile fits 64 KiB of LDS and there are enough blocks to fill
    // 256 CUs twice over; otherwise 64-row blocks.
    constexpr bool fits128 = 128 * (C * (int)sizeof(T) + 16) <= 68 * 1024;
    if constexpr (fits128) {
        if (p.M >= 128 * 512) return launch_one<T, C, 128, EP>(p, st);
    }
    return launch_one<T, C, 64, EP>(p, st);
}

template <typename T, int EP>
int launch_c(const LnGemmParams& p, int C, hipStream_t st) {
    switch (C) {
        case 16: return launch_bm<T, 16, EP>(p, st);
        case 32: return launch_bm<T, 32, EP>(p, st);
        case 64: return launch_bm<T, 64, EP>(p, st);
        case 128: return launch_bm<T, 128, EP>(p, st);
        case 256: return launch_bm<T, 256, EP>(p, st);
        case 512: return launch_bm<T, 512, EP>(p, st);
        default:
            set_error("ln_gemm: C=%d unsupported (16,32,64,128,256,512)", C);
            return UF_ERR_UNSUPPORTED;
    }
}

// ln_gemm_kernel's phase 0 as a function (the kernel above keeps its own inlined copy: routing it through this function changed its
// register allocation): normalise rows [m0, m0 + BM) of the f32 stream (gathered through the roll / partition index when `windowed`), add the
// modulator row and leave them as T in the LDS tile As (row stride SA bytes); rows past M are zero.
template <typename T, int C, int BM, int SA>
__device__ __forceinline__ void ln_rows_to_lds(char* As, const float* x, int ld, const float* gamma, const float* beta, const float* modulator, int m0, int M,
                                               int H, int W, int windowed, int shift, int tid) {
    constexpr int LPR = (C / 4) < 64 ? (C / 4) : 64;
    constexpr int V4 = C / (4 * LPR);
    constexpr int RPP = 256 / LPR;                 // rows normalised per pass of the block
    constexpr int NP = BM / RPP;                   // passes
    constexpr int U = (16 / V4) < NP ? (16 / V4) : NP;  // row groups kept in flight (16 x 16-byte loads per thread issued together)
    static_assert(NP % U == 0, "pass batching");
    const int sub = tid % LPR;
#pragma unroll 1
    for (int r0 = 0; r0 < BM; r0 += RPP * U) {
        f32x4 v[U][V4];
        bool live[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int m = m0 + r0 + u * RPP + tid / LPR;
            live[u] = m < M;
            const int mc = live[u] ? m : M - 1;   // clamped: the load itself is unconditional
            const int src = windowed ? window_row_to_token(mc, H, W, shift) : mc;
#pragma unroll
            for (int i = 0; i < V4; ++i) v[u][i] = *reinterpret_cast<const f32x4*>(x + (size_t)src * ld + (i * LPR + sub) * 4);
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
                f32x4 y = v[u][i] * rstd * *reinterpret_cast<const f32x4*>(gamma + c) + *reinterpret_cast<const f32x4*>(beta + c);
                if (modulator) y += *reinterpret_cast<const f32x4*>(modulator + (size_t)((m0 + row) & 63) * C + c);  // uniform branch
                if (!live[u]) y = f32x4{0.f, 0.f, 0.f, 0.f};
                store4(reinterpret_cast<T*>(As + row * SA) + c, y);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// ConvProjection producer (uf_ln_convqkv_fwd; reference ConvProjection / SepConv2d, model.py:344-410).  One workgroup owns ONE 8x8 window
// (64 rows).  Phase 0 is ln_gemm_kernel's and leaves the window's tile xw [64][C] in LDS, rounded to T.  Then, for each third j = q, k, v:
//   all 256 threads form P_j = ReLU(depthwise 3x3 of xw + bias) in a second LDS tile -- zero padding at the WINDOW border, so no halo; the
//   stencil, the bias and the ReLU in f32, the result rounded to T as a stored activation is -- then a barrier, then the four waves walk the
//   third's 64-column units as ln_gemm_kernel does (fragment-major weights streamed through the 3-deep ring, f32 MFMA accumulation, + f32 bias,
//   q times hd^-0.5, rounded to T, the q / k and v^T epilogues through the wave's private slab), then a barrier before P is overwritten.
// LDS: two tiles of 64 x (C sizeof(T) + 16) bytes + the four slabs: 139 KiB at C = 512 with 2-byte T, 147 KiB at C = 256 in f32.
// GXW (f32 at C = 512, where two tiles do not fit): there is no xw tile; the stencil reads xw from global memory, T[M][C] in window-row
// order, written by the windowed LayerNorm kernel in a launch of its own.
struct LnConvParams {
    const float* x; int ld;
    const float* gamma; const float* beta; const float* modulator;
    const void* xw;                     // GXW only
    const float* dw9; const float* bdw; // f32 (3,9,C), (3,C)
    const void* Wpw; const float* bpw;  // T (3C,C) fragment-major, f32 (3C)
    int M, H, W, shift;
    void* q; void* k; void* vt; int heads, hd, hd_log2; float qscale;
};

template <typename T, int C, bool GXW>
__global__ __launch_bounds__(256, (C * sizeof(T) >= 256 ? 1 : 2)) void ln_convqkv_kernel(const LnConvParams p) {
    constexpr int SZ = sizeof(T);
    constexpr int EPC = 16 / SZ;
    constexpr int SA = C * SZ + 16;               // LDS row stride of a tile
    constexpr int SS = 64 * SZ + 16;              // LDS row stride of a staging slab (16 rows x 64 values)
    constexpr int KS = (C + 31) / 32;             // MFMA k-steps
    constexpr bool SLIM = SZ == 4 && C >= 256;    // f32 (the parity mode) at the two widest tiles: a shallower pipeline, so that nothing spills
    constexpr int RING = SLIM ? 2 : 3;            // weight-fragment prefetch depth (k-steps)
    constexpr int ABUF = SLIM ? 1 : 2;            // activation-fragment buffers
    constexpr int NT = C / 16;                    // 16-column n-tiles per third
    constexpr int NU = (C + 63) / 64;             // 64-column units per third
    constexpr int VT = C >= 64 ? 4 : NT;          // n-tiles per unit (C = 16, 32: the one unit is 1 or 2 tiles wide)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Ps = smem;
    char* As = smem + 64 * SA;                    // absent with GXW
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fg = lane >> 4;
    char* stg = smem + (GXW ? 1 : 2) * 64 * SA + wave * (16 * SS);
    const int win = blockIdx.x, m0 = win * 64;

    if constexpr (!GXW) {
        ln_rows_to_lds<T, C, 64, SA>(As, p.x, p.ld, p.gamma, p.beta, p.modulator, m0, p.M, p.H, p.W, 1, p.shift, tid);
        lds_barrier();
    }
    // 4 channels of row t of xw as f32
    auto xload = [&](int t, int c) {
        using Ch = Chunk<T, 4>;
        typename Ch::Raw r;
        if constexpr (GXW) r = *reinterpret_cast<const typename Ch::Raw*>(reinterpret_cast<const T*>(p.xw) + (size_t)(m0 + t) * C + c);
        else r = *reinterpret_cast<const typename Ch::Raw*>(As + t * SA + c * SZ);
        float f[4];
        Ch::unpack(r, f);
        return f32x4{f[0], f[1], f[2], f[3]};
    };

#pragma unroll 1
    for (int j = 0; j < 3; ++j) {
        // ---------------- P_j: depthwise 3x3 inside the window + bias + ReLU -> LDS ------------------------------------------
        {
            constexpr int CG = C / 4;             // a thread keeps one group of 4 channels (its 9 taps stay in registers) ...
            constexpr int TPP = 256 / CG;         // ... and walks the window's rows TPP at a time
            const int c = (tid % CG) * 4;
            f32x4 wt[9];
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) wt[tap] = *reinterpret_cast<const f32x4*>(p.dw9 + (size_t)(j * 9 + tap) * C + c);
            const f32x4 bb = *reinterpret_cast<const f32x4*>(p.bdw + j * C + c);
#pragma unroll 2
            for (int it = 0; it < 64 / TPP; ++it) {
                const int t = tid / CG + it * TPP;
                const int y = t >> 3, x = t & 7;
                f32x4 acc = bb;
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) {
                        const int yy = y + ky - 1, xx = x + kx - 1;
                        const bool in = (unsigned)yy < 8u && (unsigned)xx < 8u;
                        f32x4 v = xload(in ? yy * 8 + xx : t, c);        // the load is unconditional (a valid row), the value selected
                        if (!in) v = f32x4{0.f, 0.f, 0.f, 0.f};
                        acc += wt[ky * 3 + kx] * v;
                    }
                acc = f32x4{fmaxf(acc[0], 0.f), fmaxf(acc[1], 0.f), fmaxf(acc[2], 0.f), fmaxf(acc[3], 0.f)};
                store4(reinterpret_cast<T*>(Ps + t * SA) + c, acc);
            }
        }
        lds_barrier();

        // ---------------- out_j = P_j Wpw_j^T + bpw_j: barrier-free walk over the third's 64-column units -------------------------
        const T* Wt = reinterpret_cast<const T*>(p.Wpw) + (size_t)j * NT * KS * 512;   // fragment-major: [n-tile][k-step][lane][8]
        const float* bias = p.bpw + j * C;
        const T* wrow[VT];
        Frag<T> wf[RING][VT];
        auto wload = [&](int ks, int slot) {
#pragma unroll
            for (int i = 0; i < VT; ++i) load_frag(wf[slot][i], wrow[i] + ks * 512);
        };
        auto unit_prefetch = [&](int u) {       // the first RING-1 k-steps of a unit's weights, issued before the previous unit's epilogue
#pragma unroll
            for (int i = 0; i < VT; ++i) wrow[i] = Wt + ((size_t)(u * 4 + i) * KS * 64 + lane) * 8;
#pragma unroll
            for (int s = 0; s < RING - 1; ++s)
                if (s < KS) wload(s, s);
        };
        if (wave < NU) unit_prefetch(wave);
#pragma unroll 1
        for (int u = wave; u < NU; u += 4) {
            const int nbase = u * 64;             // first channel of the unit within the third
            f32x4 acc[VT][4];
#pragma unroll
            for (int i = 0; i < VT; ++i)
#pragma unroll
                for (int jm = 0; jm < 4; ++jm) acc[i][jm] = f32x4{0.f, 0.f, 0.f, 0.f};
            const char* arow = Ps + fr * SA + fg * 8 * SZ;
            Frag<T> af[ABUF][4];
            auto aload = [&](int ks, int slot) {
#pragma unroll
                for (int jm = 0; jm < 4; ++jm) {
                    if (fg * 8 < C) load_frag(af[slot][jm], reinterpret_cast<const T*>(arow + jm * 16 * SA + ks * 32 * SZ));
                    else af[slot][jm].zero();     // C = 16: k-slots 16..31 are zero padding
                }
            };
            aload(0, 0);
            // the software pipeline of ln_gemm_kernel: weights for k-step ks+2 and activation fragments for ks+1 are issued before the MFMAs of ks
            auto kloop = [&](auto vt_tag) {
                constexpr bool VTR = decltype(vt_tag)::value;   // V tiles are computed transposed (lane = channel, 4 consecutive tokens)
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    if (ks + RING - 1 < KS) wload(ks + RING - 1, (ks + RING - 1) % RING);
                    if (ABUF == 2 && ks + 1 < KS) aload(ks + 1, (ks + 1) & 1);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int i = 0; i < VT; ++i)
#pragma unroll
                        for (int jm = 0; jm < 4; ++jm) {
                            if constexpr (VTR) mma16(acc[i][jm], af[ks % ABUF][jm], wf[ks % RING][i]);
                            else mma16(acc[i][jm], wf[ks % RING][i], af[ks % ABUF][jm]);
                        }
                    __builtin_amdgcn_sched_barrier(0);
                    if (ABUF == 1 && ks + 1 < KS) aload(ks + 1, 0);
                }
            };
            if (j == 2) kloop(std::true_type{});
            else kloop(std::false_type{});
            if (u + 4 < NU) unit_prefetch(u + 4);
            __builtin_amdgcn_sched_barrier(0);

            constexpr int CPR = 64 * SZ / 16;         // 16-byte chunks per staged row
            constexpr int ITERS = 16 * CPR / 64;
            if (j < 2) {
                // ---- q, k: [token][channel] tiles, one 16-row m-tile per pass through the wave's slab; channel n of the third = head n / hd, d = n % hd
                T* dst0 = reinterpret_cast<T*>(j == 0 ? p.q : p.k) + (size_t)win * p.heads * 64 * p.hd;
                f32x4 bv[VT];
#pragma unroll
                for (int i = 0; i < VT; ++i) bv[i] = *reinterpret_cast<const f32x4*>(bias + nbase + i * 16 + fg * 4);
#pragma unroll
                for (int jm = 0; jm < 4; ++jm) {
#pragma unroll
                    for (int i = 0; i < VT; ++i) {
                        f32x4 v = acc[i][jm] + bv[i];
                        if (j == 0) v *= p.qscale;          // q = q * scale (model.py:497)
                        store4(reinterpret_cast<T*>(stg + fr * SS) + i * 16 + fg * 4, v);
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
                    for (int it = 0; it < ITERS; ++it) {
                        const int idx = it * 64 + lane;
                        const int r = idx / CPR, cb = idx % CPR;
                        if (cb * EPC < VT * 16) {
                            const int n = nbase + cb * EPC;
                            const u32x4 val = *reinterpret_cast<const u32x4*>(stg + r * SS + cb * 16);
                            T* dst = dst0 + ((size_t)(n >> p.hd_log2) * 64 + jm * 16 + r) * p.hd + (n & (p.hd - 1));
                            *reinterpret_cast<u32x4*>(dst) = val;
                        }
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                }
            } else {
                // ---- v^T: [channel][token] tiles, one 16-channel n-tile per pass
                T* dst0 = reinterpret_cast<T*>(p.vt) + (size_t)win * p.heads * p.hd * 64;
#pragma unroll
                for (int i = 0; i < VT; ++i) {
                    const float b = bias[nbase + i * 16 + fr];
#pragma unroll
                    for (int jm = 0; jm < 4; ++jm) {
                        const f32x4 v = {acc[i][jm][0] + b, acc[i][jm][1] + b, acc[i][jm][2] + b, acc[i][jm][3] + b};
                        store4(reinterpret_cast<T*>(stg + fr * SS) + jm * 16 + fg * 4, v);
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
                    for (int it = 0; it < ITERS; ++it) {
                        const int idx = it * 64 + lane;
                        const int r = idx / CPR, cb = idx % CPR;
                        const int n = nbase + i * 16 + r;       // channel of the third = head * hd + d: row (head, d) of v^T
                        const u32x4 val = *reinterpret_cast<const u32x4*>(stg + r * SS + cb * 16);
                        *reinterpret_cast<u32x4*>(dst0 + (size_t)n * 64 + cb * EPC) = val;
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                }
            }
        }
        lds_barrier();      // every wave is done with P_j before the next third overwrites it
    }
}

template <typename T, int C>
int launch_convqkv(LnConvParams p, hipStream_t st) {
    constexpr int SZ = sizeof(T);
    constexpr int slabs = 4 * 16 * (64 * SZ + 16), tile = 64 * (C * SZ + 16);
    constexpr bool GXW = 2 * tile + slabs > 160 * 1024;      // f32 at C = 512
    static_assert(!GXW || std::is_same<T, float>::value, "only f32 at C = 512 reads xw from global memory");
    constexpr int smem = (GXW ? 1 : 2) * tile + slabs;
    static_assert(smem <= 160 * 1024, "LDS budget");
    auto kern = ln_convqkv_kernel<T, C, GXW>;
    static bool lds_done[64] = {};
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), smem, lds_done, "ln_convqkv")) return rc;
    if constexpr (GXW) {
        // xw goes through global memory: window w's tile lands in ITS OWN 64 C elements of vt, which only that window's workgroup reads, and
        // overwrites last (the v^T epilogue runs behind the barrier that ends the P_v stencil)
        if (int rc = launch_layernorm(p.x, p.ld, p.gamma, p.beta, p.modulator, p.vt, p.M, p.H, p.W, C, 1, p.shift, UF_F32, st)) return rc;
        p.xw = p.vt;
    }
    char name[96] = "";
    if (timing_enabled()) snprintf(name, sizeof(name), "ln_convqkv_%s_c%d %dx%dx%d", TypeName<T>::s, C, p.M, 3 * C, C);
    {
        ScopedTimer tm(name, 2.0 * p.M * 3 * C * C + 2.0 * 27 * p.M * C, (double)p.M * C * 4 + 3.0 * C * C * SZ + 3.0 * p.M * C * SZ, st);
        hipLaunchKernelGGL(kern, dim3(p.M / 64), dim3(256), smem, st, p);
    }
    return check_launch("ln_convqkv");
}

template <typename T>
int launch_convqkv_c(const LnConvParams& p, int C, hipStream_t st) {
    switch (C) {
        case 16: return launch_convqkv<T, 16>(p, st);
        case 32: return launch_convqkv<T, 32>(p, st);
        case 64: return launch_convqkv<T, 64>(p, st);
        case 128: return launch_convqkv<T, 128>(p, st);
        case 256: return launch_convqkv<T, 256>(p, st);
        case 512: return launch_convqkv<T, 512>(p, st);
        default:
            set_error("uf_ln_convqkv_fwd: C=%d unsupported (16,32,64,128,256,512)", C);
            return UF_ERR_UNSUPPORTED;
    }
}

int check_common(const float* x, int ld, const float* g, const float* b, const void* w, const float* bias, int B, int H, int W, int C,
                 int windowed, uf_dtype dtype) {
    UF_REQUIRE(x && g && b && w && bias, UF_ERR_NULL, "ln_gemm: null pointer");
    UF_REQUIRE(B > 0 && H > 0 && W > 0, UF_ERR_SHAPE, "ln_gemm: B=%d H=%d W=%d", B, H, W);
    UF_REQUIRE(!windowed || (H % 8 == 0 && W % 8 == 0), UF_ERR_SHAPE, "ln_gemm: windowed needs H,W multiples of 8");
    UF_REQUIRE(ld >= C && ld % 4 == 0, UF_ERR_ALIGN, "ln_gemm: ld=%d", ld);
    UF_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)w % 16) == 0 && ((uintptr_t)bias % 16) == 0, UF_ERR_ALIGN, "ln_gemm: operands must be 16-byte aligned");
    UF_REQUIRE(dtype_ok(dtype), UF_ERR_UNSUPPORTED, "ln_gemm: dtype %d", (int)dtype);
    return UF_OK;
}

}  // namespace
}  // namespace uf

using namespace uf;

extern "C" int uf_ln_qkv_fwd(const float* x, int ld, const float* gamma, const float* beta, const float* modulator,
                             const void* Wqkv, const float* bqkv, void* q, void* k, void* vt, int B, int H, int W, int C,
                             int heads, int shift, uf_dtype dtype, void* stream) {
    int rc = check_common(x, ld, gamma, beta, Wqkv, bqkv, B, H, W, C, 1, dtype);
    if (rc) return rc;
    UF_REQUIRE(q && k && vt, UF_ERR_NULL, "uf_ln_qkv_fwd: null output");
    UF_REQUIRE(heads > 0 && C % heads == 0, UF_ERR_SHAPE, "uf_ln_qkv_fwd: C=%d heads=%d", C, heads);
    const int hd = C / heads;
    UF_REQUIRE(hd == 16 || hd == 32 || hd == 64, UF_ERR_UNSUPPORTED, "uf_ln_qkv_fwd: head_dim %d (16, 32 or 64 supported)", hd);
    UF_REQUIRE(shift >= 0 && shift < 8, UF_ERR_SHAPE, "uf_ln_qkv_fwd: shift=%d", shift);
    LnGemmParams p{};
    p.x = x; p.ld = ld; p.gamma = gamma; p.beta = beta; p.modulator = modulator; p.Wt = Wqkv; p.bias = bqkv;
    p.M = B * H * W; p.N = 3 * C; p.H = H; p.W = W; p.windowed = 1; p.shift = shift;
    p.q = q; p.k = k; p.vt = vt; p.heads = heads; p.hd = hd; p.qscale = (float)(1.0 / sqrt((double)hd));
    hipStream_t st = (hipStream_t)stream;
    if (dtype == UF_BF16) return launch_c<bf16, EP_QKV>(p, C, st);
    if (dtype == UF_F16) return launch_c<f16, EP_QKV>(p, C, st);
    return launch_c<float, EP_QKV>(p, C, st);
}

extern "C" int uf_ln_convqkv_fwd(const float* x, int ld, const float* gamma, const float* beta, const float* modulator, const float* dw9,
                                 const float* bdw, const void* Wpw_fm, const float* bpw, void* q, void* k, void* vt, int B, int H, int W, int C,
                                 int heads, int shift, uf_dtype dtype, void* stream) {
    int rc = check_common(x, ld, gamma, beta, Wpw_fm, bpw, B, H, W, C, 1, dtype);
    if (rc) return rc;
    UF_REQUIRE(dw9 && bdw && q && k && vt, UF_ERR_NULL, "uf_ln_convqkv_fwd: null pointer");
    UF_REQUIRE(C == 16 || C == 32 || C == 64 || C == 128 || C == 256 || C == 512, UF_ERR_UNSUPPORTED, "uf_ln_convqkv_fwd: C=%d unsupported (16,32,64,128,256,512)", C);
    UF_REQUIRE(heads > 0 && C % heads == 0, UF_ERR_SHAPE, "uf_ln_convqkv_fwd: C=%d heads=%d", C, heads);
    const int hd = C / heads;
    UF_REQUIRE(hd == 16 || hd == 32 || hd == 64, UF_ERR_UNSUPPORTED, "uf_ln_convqkv_fwd: head_dim %d (16, 32 or 64 supported)", hd);
    UF_REQUIRE(shift >= 0 && shift < 8, UF_ERR_SHAPE, "uf_ln_convqkv_fwd: shift=%d", shift);
    UF_REQUIRE((long long)B * H * W * (long long)C < 0x7fffffffLL, UF_ERR_SHAPE, "uf_ln_convqkv_fwd: tensor too large for 32-bit indexing");
    const uintptr_t al = (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)modulator | (uintptr_t)dw9 | (uintptr_t)bdw | (uintptr_t)q | (uintptr_t)k | (uintptr_t)vt;
    UF_REQUIRE((al % 16) == 0, UF_ERR_ALIGN, "uf_ln_convqkv_fwd: operands must be 16-byte aligned");
    LnConvParams p{};
    p.x = x; p.ld = ld; p.gamma = gamma; p.beta = beta; p.modulator = modulator; p.dw9 = dw9; p.bdw = bdw; p.Wpw = Wpw_fm; p.bpw = bpw;
    p.M = B * H * W; p.H = H; p.W = W; p.shift = shift;
    p.q = q; p.k = k; p.vt = vt; p.heads = heads; p.hd = hd; p.hd_log2 = hd == 16 ? 4 : (hd == 32 ? 5 : 6); p.qscale = (float)(1.0 / sqrt((double)hd));
    hipStream_t st = (hipStream_t)stream;
    if (dtype == UF_BF16) return launch_convqkv_c<bf16>(p, C, st);
    if (dtype == UF_F16) return launch_convqkv_c<f16>(p, C, st);
    return launch_convqkv_c<float>(p, C, st);
}

extern "C" int uf_ln_linear_gelu_fwd(const float* x, int ld, const float* gamma, const float* beta, const void* W1,
                                     const float* b1, void* out, int M, int N, int C, uf_dtype dtype, void* stream) {
    int rc = check_common(x, ld, gamma, beta, W1, b1, 1, 1, M > 0 ? M : 1, C, 0, dtype);
    if (rc) return rc;
    UF_REQUIRE(out && M > 0 && N > 0, UF_ERR_NULL, "uf_ln_linear_gelu_fwd: bad output / shape");
    UF_REQUIRE(N % (dtype_half(dtype) ? 8 : 4) == 0, UF_ERR_SHAPE, "uf_ln_linear_gelu_fwd: N=%d", N);
    LnGemmParams p{};
    p.x = x; p.ld = ld; p.gamma = gamma; p.beta = beta; p.modulator = nullptr; p.Wt = W1; p.bias = b1;
    p.M = M; p.N = N; p.H = 1; p.W = M; p.windowed = 0; p.shift = 0; p.out = out; p.ldo = N;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == UF_BF16) return launch_c<bf16, EP_GELU>(p, C, st);
    if (dtype == UF_F16) return launch_c<f16, EP_GELU>(p, C, st);
    return launch_c<float, EP_GELU>(p, C, st);
}
