// HBM-bound kernels of the LeWin block: index-only window ops, LayerNorm(+roll+partition+
// modulator), the LeFF depthwise 3x3 + GELU stencil, and the 3-channel stem/head convolutions.
// All of them move 16 bytes per lane per access and keep consecutive lanes on consecutive
// addresses of the channel-last token layout.
#include "uf_internal.h"

namespace uf {
namespace {

// ---------------------------------------------------------------------------------------
// a1-a3: window_partition / window_reverse with the cyclic shift folded into the index.
// One thread moves one 16-byte chunk of a token row (bit-exact copy).
// ---------------------------------------------------------------------------------------
template <bool REVERSE>
__global__ void window_copy_kernel(const u32x4* __restrict__ src, u32x4* __restrict__ dst, int rows, int chunks_per_row,
                                   int H, int W, int shift) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)rows * chunks_per_row) return;
    const int m = (int)(idx / chunks_per_row), c = (int)(idx - (long long)m * chunks_per_row);
    const int tok = window_row_to_token(m, H, W, shift);
    if (REVERSE) dst[(size_t)tok * chunks_per_row + c] = src[(size_t)m * chunks_per_row + c];
    else dst[(size_t)m * chunks_per_row + c] = src[(size_t)tok * chunks_per_row + c];
}

// generic fall-back for rows that are not a multiple of 16 bytes (element granularity)
template <bool REVERSE, typename E>
__global__ void window_copy_elem_kernel(const E* __restrict__ src, E* __restrict__ dst, int rows, int C, int H, int W, int shift) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)rows * C) return;
    const int m = (int)(idx / C), c = (int)(idx - (long long)m * C);
    const int tok = window_row_to_token(m, H, W, shift);
    if (REVERSE) dst[(size_t)tok * C + c] = src[(size_t)m * C + c];
    else dst[(size_t)m * C + c] = src[(size_t)tok * C + c];
}

// ---------------------------------------------------------------------------------------
// a5/a6: LayerNorm over C (+ roll + partition gather + modulator add), f32 in, T out.
// LPR lanes share one row, each lane owns C/LPR values (4 or 8) in registers; two-pass
// (mean, then centred variance) like ATen's native_layer_norm; xor-shuffle reductions.
// ---------------------------------------------------------------------------------------
template <typename T, int C>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, int ld_x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, const float* __restrict__ modulator,
                                                        T* __restrict__ out, int rows, int H, int W, int windowed, int shift) {
    constexpr int LPR = (C / 4) < 64 ? (C / 4) : 64;  // lanes per row
    constexpr int V4 = C / (4 * LPR);                 // float4 per lane (1 or 2)
    constexpr int RPB = 256 / LPR;                    // rows per block
    const int sub = threadIdx.x % LPR;
    const int m = blockIdx.x * RPB + threadIdx.x / LPR;
    const bool live = m < rows;
    const int mc = live ? m : rows - 1;   // clamped so that the loads below are unconditional
    const int src = windowed ? window_row_to_token(mc, H, W, shift) : mc;
    f32x4 v[V4];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < V4; ++i) {
        v[i] = *reinterpret_cast<const f32x4*>(x + (size_t)src * ld_x + (i * LPR + sub) * 4);
        sum += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
    }
    sum = allreduce<RedSum, LPR>(sum);
    const float mean = sum * (1.0f / C);
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < V4; ++i) {
        v[i] -= mean;
        sq += (v[i][0] * v[i][0] + v[i][1] * v[i][1]) + (v[i][2] * v[i][2] + v[i][3] * v[i][3]);
    }
    sq = allreduce<RedSum, LPR>(sq);
    const float rstd = 1.0f / sqrtf(sq * (1.0f / C) + 1e-5f);
    if (!live) return;
#pragma unroll
    for (int i = 0; i < V4; ++i) {
        const int c = (i * LPR + sub) * 4;
        const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + c);
        const f32x4 b = *reinterpret_cast<const f32x4*>(beta + c);
        f32x4 y = v[i] * rstd * g + b;
        if (modulator) y += *reinterpret_cast<const f32x4*>(modulator + (size_t)(m & 63) * C + c);  // model.py:966-969
        store4(out + (size_t)m * C + c, y);
    }
}

// ---------------------------------------------------------------------------------------
// a10: depthwise 3x3 (zero pad 1) + bias + erf-GELU on [B][H][W][C] (LeFF, model.py:659-660).
// One thread = one pixel x VEC channels (16 bytes of T); fp32 accumulate.
// ---------------------------------------------------------------------------------------
template <typename T> struct Vec16 {   // the 2-byte operand types (bf16, f16)
    static_assert(sizeof(T) == 2, "2-byte operand type");
    static constexpr int N = 8;
    static __device__ __forceinline__ void load(const T* p, float* f) { unpack8<T>(*reinterpret_cast<const u32x4*>(p), f); }
    static __device__ __forceinline__ void store(T* p, const float* f) { *reinterpret_cast<u32x4*>(p) = pack8<T>(f); }
};
template <> struct Vec16<float> {
    static constexpr int N = 4;
    static __device__ __forceinline__ void load(const float* p, float* f) {
        const f32x4 r = *reinterpret_cast<const f32x4*>(p);
        f[0] = r[0]; f[1] = r[1]; f[2] = r[2]; f[3] = r[3];
    }
    static __device__ __forceinline__ void store(float* p, const float* f) {
        *reinterpret_cast<f32x4*>(p) = f32x4{f[0], f[1], f[2], f[3]};
    }
};

// One thread = a vertical strip of DW_R output pixels x VEC channels: each input vector is loaded
// once per (column tap) and feeds up to 3 output rows, the 3 column-tap weights live in registers.
constexpr int DW_R = 4;

// round N values to the operand type and back (what a later pass would read from memory)
template <typename T, int N> __device__ __forceinline__ void round_to(float* f) {
    if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int i = 0; i < N; i += 2) {
            unpack2<T>(pack2<T>(f[i], f[i + 1]), f[i], f[i + 1]);
        }
    }
}

// ACT 0: the bare stencil (also the backward: flipped taps);  1: + GELU (the LeFF forward);  2: out = pre-activation AND aux = GELU of
// it as stored (training forward keeps both);  3: out = stencil (as stored) * GELU'(aux) (input gradient through the preceding GELU)
template <typename T, int ACT>
__global__ __launch_bounds__(256) void dwconv3x3_gelu_kernel(const T* __restrict__ x, const float* __restrict__ w9,
                                                             const float* __restrict__ bias, T* __restrict__ out, T* __restrict__ aux, int B, int H,
                                                             int W, int C) {
    constexpr int N = Vec16<T>::N;
    const int cv = C / N;
    const int strips = H / DW_R;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)B * strips * W * cv) return;
    const int c = (int)(idx % cv) * N;
    long long rest = idx / cv;
    const int xw = (int)(rest % W); rest /= W;
    const int y0 = (int)(rest % strips) * DW_R;
    const int b = (int)(rest / strips);
    float acc[DW_R][N];
#pragma unroll
    for (int r = 0; r < DW_R; ++r)
#pragma unroll
        for (int i = 0; i < N; i += 4) {    // 16-byte loads (C % 4 == 0): as dword loads the per-lane 32-byte stride made every tap-weight load touch 16 cache lines,
            const f32x4 bv = bias ? *reinterpret_cast<const f32x4*>(bias + c + i) : f32x4{0.f, 0.f, 0.f, 0.f};   // 80 such loads per thread against 18 data loads
            acc[r][i] = bv[0]; acc[r][i + 1] = bv[1]; acc[r][i + 2] = bv[2]; acc[r][i + 3] = bv[3];
        }
    const T* xb = x + (size_t)b * H * W * C + c;
    float auxf[ACT == 3 ? DW_R : 1][N];     // ACT 3: the pre-activations of this thread's outputs, requested before the tap loop
    if constexpr (ACT == 3) {
#pragma unroll
        for (int r = 0; r < DW_R; ++r) Vec16<T>::load(aux + ((size_t)(b * H + y0 + r) * W + xw) * C + c, auxf[r]);
    }
    // one column tap at a time (not unrolled): fully unrolled, hipcc hoists all 18 loads and 72 tap weights, 208-234 VGPRs = 2
    // waves per SIMD, and the kernel ran at 2 TB/s; with 6 loads in flight per thread it fits 4-5 waves
#pragma unroll 1
    for (int kx = 0; kx < 3; ++kx) {
        // zero padding without guarded loads (a guarded load costs an exec-masked branch and a
        // vmcnt(0) wait): coordinates are clamped and the column / row masks are folded into the
        // weights / the loaded values.
        const int ixr = xw + kx - 1;
        const float mx = (ixr >= 0 && ixr < W) ? 1.0f : 0.0f;
        const int ix = ixr < 0 ? 0 : (ixr >= W ? W - 1 : ixr);
        float wk[3][N];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int i = 0; i < N; i += 4) {
                const f32x4 wv = *reinterpret_cast<const f32x4*>(w9 + (size_t)(ky * 3 + kx) * C + c + i);
                wk[ky][i] = wv[0] * mx; wk[ky][i + 1] = wv[1] * mx; wk[ky][i + 2] = wv[2] * mx; wk[ky][i + 3] = wv[3] * mx;
            }
#pragma unroll
        for (int r = -1; r <= DW_R; ++r) {   // input row y0 + r feeds output rows r+1-ky
            const int iyr = y0 + r;
            const bool rowok = iyr >= 0 && iyr < H;
            const int iy = iyr < 0 ? 0 : (iyr >= H ? H - 1 : iyr);
            float f[N];
            Vec16<T>::load(xb + ((size_t)iy * W + ix) * C, f);
            if constexpr (ACT == 4) {     // the input is the PRE-activation of the GELU in front of the convolution: activate as a stored T would read
                gelu_n<T, N>(f);
                round_to<T, N>(f);
            }
            if (r == -1 || r == DW_R) {   // only the halo rows can fall outside the image
#pragma unroll
                for (int i = 0; i < N; ++i) f[i] = rowok ? f[i] : 0.0f;
            }
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int orow = r + 1 - ky;
                if (orow < 0 || orow >= DW_R) continue;
#pragma unroll
                for (int i = 0; i < N; ++i) acc[orow][i] = fmaf(f[i], wk[ky][i], acc[orow][i]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < DW_R; ++r) {
        const size_t o = ((size_t)(b * H + y0 + r) * W + xw) * C + c;
        if constexpr (ACT == 1) gelu_n<T, N>(acc[r]);
        if constexpr (ACT == 3) {
            round_to<T, N>(acc[r]);
#pragma unroll
            for (int i = 0; i < N; ++i) acc[r][i] *= gelu_grad_t<T>(auxf[r][i]);
        }
        Vec16<T>::store(out + o, acc[r]);
        if constexpr (ACT == 2 || ACT == 4) {
            round_to<T, N>(acc[r]);
            gelu_n<T, N>(acc[r]);
            Vec16<T>::store(aux + o, acc[r]);
        }
    }
}

// The same stencil (ACT 0, 1, 2) WALKING along x.  The kernel above gives a thread one pixel column: each input vector is then requested
// by the threads of three neighbouring columns, i.e. three different waves, and with the one-tap timing ablation (profiles/
// r03_kx_abl.txt) it ran at 5.3-5.9 TB/s against 3.4-3.9 TB/s: the 3x re-read through L1 / L2 was the limit, not HBM.  Here a thread
// owns 4 channels x a strip of DW_R rows x SEG consecutive pixel columns and keeps the last three input columns ((DW_R + 2) rows
// each) in registers as f32: every step loads ONE new column (6 x 8 bytes for the 2-byte types), so an input element is loaded
// (SEG + 2) / SEG x 1.5 times instead of 4.5.  4 channels, not 8: 72 column + 36 tap + 16 accumulator registers leave 4 waves / SIMD.
// Same FMA order per output as the kernel above (column taps outermost, then rows): bit-identical results.
template <typename T, int ACT, int SEG>
__global__ __launch_bounds__(256) void dwconv3x3_walk_kernel(const T* __restrict__ x, const float* __restrict__ w9, const float* __restrict__ bias,
                                                             T* __restrict__ out, T* __restrict__ aux, int B, int H, int W, int C) {
    constexpr int N = 4, R = DW_R;
    using CH = Chunk<T, N>;
    using Raw = typename CH::Raw;
    const int cv = C / N, strips = H / R, segs = W / SEG;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)B * strips * segs * cv) return;
    const int c = (int)(idx % cv) * N;
    long long rest = idx / cv;
    const int x0 = (int)(rest % segs) * SEG; rest /= segs;
    const int y0 = (int)(rest % strips) * R;
    const int b = (int)(rest / strips);
    f32x4 wt[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) wt[t] = *reinterpret_cast<const f32x4*>(w9 + (size_t)t * C + c);
    const f32x4 bv = bias ? *reinterpret_cast<const f32x4*>(bias + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    // 32-bit byte offsets from the tensor base (the launcher checks the tensor is under 4 GiB); halo rows clamped into the image, masked
    const unsigned pixb = (unsigned)C * (unsigned)sizeof(T), rowb = (unsigned)W * pixb;
    const unsigned o00 = ((unsigned)(b * H + y0) * W + x0) * pixb + (unsigned)c * (unsigned)sizeof(T);
    unsigned ro[R + 2];
    ro[0] = y0 > 0 ? o00 - rowb : o00;
#pragma unroll
    for (int r = 0; r < R; ++r) ro[r + 1] = o00 + r * rowb;
    ro[R + 1] = y0 + R < H ? o00 + R * rowb : o00 + (R - 1) * rowb;
    const float mtop = y0 > 0 ? 1.0f : 0.0f, mbot = y0 + R < H ? 1.0f : 0.0f;
    const char* xb = reinterpret_cast<const char*>(x);
    char* ob = reinterpret_cast<char*>(out);
    char* ab = reinterpret_cast<char*>(aux);

    float col[3][R + 2][N];        // input columns xx - 1, xx, xx + 1 of the current output column xx, rotating
    auto load_col = [&](float (&cl)[R + 2][N], int dx, float m) {      // column x0 + dx (clamped by the caller), times the column mask m
        Raw raw[R + 2];
#pragma unroll
        for (int r = 0; r < R + 2; ++r) raw[r] = *reinterpret_cast<const Raw*>(xb + (ro[r] + (unsigned)(dx * (int)pixb)));
#pragma unroll
        for (int r = 0; r < R + 2; ++r) {
            CH::unpack(raw[r], cl[r]);
            if constexpr (ACT == 4) {     // pre-activation in, GELU applied here (rounded as the stored activation was): linear1 need not write it
                gelu_n<T, N>(cl[r]);
                round_to<T, N>(cl[r]);
            }
            const float mr = (r == 0 ? mtop : (r == R + 1 ? mbot : 1.0f)) * m;
            if (r == 0 || r == R + 1) {
#pragma unroll
                for (int i = 0; i < N; ++i) cl[r][i] *= mr;
            } else if (m != 1.0f) {
#pragma unroll
                for (int i = 0; i < N; ++i) cl[r][i] *= m;
            }
        }
    };
    auto emit = [&](const float (&cL)[R + 2][N], const float (&cM)[R + 2][N], const float (&cR)[R + 2][N], int dx) {
        float acc[R][N];
#pragma unroll
        for (int r = 0; r < R; ++r) { acc[r][0] = bv[0]; acc[r][1] = bv[1]; acc[r][2] = bv[2]; acc[r][3] = bv[3]; }
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const float (&cl)[R + 2][N] = kx == 0 ? cL : (kx == 1 ? cM : cR);
#pragma unroll
            for (int r = -1; r <= R; ++r)
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) {
                    const int orow = r + 1 - ky;
                    if (orow < 0 || orow >= R) continue;
#pragma unroll
                    for (int i = 0; i < N; ++i) acc[orow][i] = fmaf(cl[r + 1][i], wt[ky * 3 + kx][i], acc[orow][i]);
                }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const unsigned o = ro[r + 1] + (unsigned)(dx * (int)pixb);
            if constexpr (ACT == 1) gelu_n<T, N>(acc[r]);
            *reinterpret_cast<Raw*>(ob + o) = CH::pack(acc[r]);
            if constexpr (ACT == 2 || ACT == 4) {
                round_to<T, N>(acc[r]);
                gelu_n<T, N>(acc[r]);
                *reinterpret_cast<Raw*>(ab + o) = CH::pack(acc[r]);
            }
        }
    };
    load_col(col[0], x0 > 0 ? -1 : 0, x0 > 0 ? 1.0f : 0.0f);
    load_col(col[1], 0, 1.0f);
    const bool last_seg = x0 + SEG >= W;
#pragma unroll 1
    for (int xs = 0; xs < SEG; xs += 3) {          // three steps per turn: the column registers rotate by name
        {
            const bool edge = last_seg && xs + 1 >= SEG;
            load_col(col[2], edge ? xs : xs + 1, edge ? 0.0f : 1.0f);
            emit(col[0], col[1], col[2], xs);
        }
        if (xs + 1 < SEG) {
            const bool edge = last_seg && xs + 2 >= SEG;
            load_col(col[0], edge ? xs + 1 : xs + 2, edge ? 0.0f : 1.0f);
            emit(col[1], col[2], col[0], xs + 1);
        }
        if (xs + 2 < SEG) {
            const bool edge = last_seg && xs + 3 >= SEG;
            load_col(col[1], edge ? xs + 2 : xs + 3, edge ? 0.0f : 1.0f);
            emit(col[2], col[0], col[1], xs + 2);
        }
    }
}

// ---------------------------------------------------------------------------------------
// a12: InputProj conv3x3(Cin->E) + LeakyReLU(0.01), NCHW image -> token rows (model.py:853-866).
// A thread owns 4 output channels x IP_PX horizontally adjacent pixels: the 27 weight vectors are loaded
// once per strip and each image row segment (IP_PX + 2 values) feeds 3 taps x IP_PX pixels, so the kernel
// issues 81 loads per 432 FMAs instead of 54 per 108.  Loads are unconditional (clamped), zero padding by
// select.  The E/4 lanes of a pixel write one contiguous token row.
// ---------------------------------------------------------------------------------------
constexpr int IP_PX_DEFAULT = 4;
template <int IP_PX>
__global__ __launch_bounds__(256) void input_proj_kernel(const float* __restrict__ img, const float* __restrict__ w27,
                                                         const float* __restrict__ bias, float* __restrict__ out, int ld_o, int B,
                                                         int Cin, int H, int W, int E) {
    // grid: x = (pixel strip, channel group) of one image row, y = row, z = image -- no 64-bit index divisions
    const unsigned eg = E / 4, xg = (W + IP_PX - 1) / IP_PX;
    const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= xg * eg) return;
    const int e = (int)(idx % eg) * 4, x0 = (int)(idx / eg) * IP_PX;
    const int yh = blockIdx.y, b = blockIdx.z;
    const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + e);
    f32x4 acc[IP_PX];
#pragma unroll
    for (int q = 0; q < IP_PX; ++q) acc[q] = bv;
    // clamped column offsets + 0/1 masks once per strip: loads stay unconditional (a select on the loaded value makes
    // hipcc sink the load into an exec-masked branch with its own s_waitcnt), 32-bit element offsets
    int xo[IP_PX + 2];
    float mx[IP_PX + 2];
#pragma unroll
    for (int q = 0; q < IP_PX + 2; ++q) {
        const int ixr = x0 + q - 1;
        xo[q] = ixr < 0 ? 0 : (ixr >= W ? W - 1 : ixr);
        mx[q] = (ixr >= 0 && ixr < W) ? 1.0f : 0.0f;
    }
    const float* wp = w27 + e;
    for (int ci = 0; ci < Cin; ++ci) {
        const float* plane = img + (b * Cin + ci) * (H * W);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iyr = yh + ky - 1;
            const float my = (iyr >= 0 && iyr < H) ? 1.0f : 0.0f;
            const float* row = plane + (iyr < 0 ? 0 : (iyr >= H ? H - 1 : iyr)) * W;
            float v[IP_PX + 2];
#pragma unroll
            for (int q = 0; q < IP_PX + 2; ++q) v[q] = row[xo[q]] * (mx[q] * my);
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const f32x4 wv = *reinterpret_cast<const f32x4*>(wp + (ci * 9 + ky * 3 + kx) * E);
#pragma unroll
                for (int q = 0; q < IP_PX; ++q) acc[q] += v[q + kx] * wv;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < IP_PX; ++q) {
        if (x0 + q >= W) break;
        f32x4 a = acc[q];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = a[i] >= 0.f ? a[i] : 0.01f * a[i];
        *reinterpret_cast<f32x4*>(out + (size_t)((b * H + yh) * W + x0 + q) * ld_o + e) = a;
    }
}

// ---------------------------------------------------------------------------------------
// a12, second form (round 4): the same convolution with the image tile staged in LDS.  The first form issues 81 global
// loads (54 of them 4-byte broadcast loads) per 432 FMAs and measured 1.1 TB/s of its 134 MB output (123 us at 16 x 256 x 256,
// profiles/r03_kernels_hip_events.json) -- bound by its own load instructions, not by the store stream.  Here a workgroup owns 4 image
// rows x TW pixels: the (4 + 2) x (TW + 2) x Cin input halo (zero-padded at the image border) goes to LDS once, coalesced; a thread owns
// 4 output channels x a strip of 8 horizontally adjacent pixels and reads per (channel, row) its 10 input values as three vector LDS
// reads and per tap one 16-byte weight vector from global memory (L1-resident: 3.4 KB shared by every thread): 27 LDS reads + 27 vector
// loads per 432 x 2 packed FMAs instead of 81 loads (54 of them 4-byte broadcasts) per 216.  The E/4 lanes of a pixel still write one contiguous token row.  Same products in the same order as the first form
// (accumulation starts at the bias, channels outer, rows, then taps): bit-identical results (tests/test_gpu_ops.py).
// ---------------------------------------------------------------------------------------
// Why every pixel value is moved into a register of its own below: hipcc had compiled `acc[q] += v[q + kx] * wv` into `v_pk_fma_f32 ... op_sel:[0,1,0]`,
// a packed-f32 operand-select form that returns a wrong low result in lanes 48-63 about once in 1e7 when an MFMA of another wave is in flight on the SIMD,
// so the side-stream images of the model's two half-batch streams came out wrong (tests/test_gpu_model.py:136).  With the moves only the clean
// `op_sel_hi:[1,0,1]` broadcast form is generated: 0 wrong outputs in 210 co-run launches (profiles/r04_run18.txt).
__global__ void empty_kernel() {}
// CIN = dd_in of the model (3 for RGB; 1, 2, 4, 6 for raw planes, packed Bayer, image + map, dual-pixel pairs): it sizes the LDS tile
// [CIN][6][RS] (at most 6 x 6 x 132 floats) and the trip count of the channel loop, nothing else.
template <int EG, int CIN>                          // lanes per pixel = E / 4 (8 for E = 32, 4 for E = 16)
__global__ __launch_bounds__(256, 4) void input_proj2_kernel(const float* __restrict__ img, const float* __restrict__ w27, const float* __restrict__ bias,
                                                          float* __restrict__ out, int ld_o, int B, int H, int W) {
    constexpr int E = EG * 4, SL = 8, NSTRIP = 64 / EG, TW = NSTRIP * SL, RS = TW + 4;     // row stride in floats (16-byte multiple; index j = pixel x0 - 1 + j)
    __shared__ __attribute__((aligned(16))) float Is[CIN][6][RS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * 4, b = blockIdx.z;
    for (int i = tid; i < CIN * 6 * (TW + 2); i += 256) {
        const int j = i % (TW + 2), r = (i / (TW + 2)) % 6, ci = i / ((TW + 2) * 6);
        const int ix = x0 - 1 + j, iy = y0 - 1 + r;
        const bool ok = ix >= 0 && ix < W && iy >= 0 && iy < H;
        const float v = img[(size_t)((b * CIN + ci) * H + (ok ? iy : 0)) * W + (ok ? ix : 0)];
        Is[ci][r][j] = ok ? v : 0.0f;
    }
    __syncthreads();
    const int e = (lane % EG) * 4, strip = lane / EG;
    const int yh = y0 + wave, xs = x0 + strip * SL;
    if (yh >= H || xs >= W) return;
    const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + e);
    f32x4 acc[SL];
#pragma unroll
    for (int q = 0; q < SL; ++q) acc[q] = bv;
#pragma unroll 1
    for (int ci = 0; ci < CIN; ++ci) {
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const float* row = &Is[ci][wave + ky][strip * SL];
            const f32x4 a0 = *reinterpret_cast<const f32x4*>(row), a1 = *reinterpret_cast<const f32x4*>(row + 4);
            const f32x2_t a2 = *reinterpret_cast<const f32x2_t*>(row + 8);
            float v[SL + 2] = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3], a2[0], a2[1]};
#pragma unroll
            for (int k = 0; k < SL + 2; ++k) asm volatile("v_mov_b32 %0, %1" : "=v"(v[k]) : "v"(v[k]));       // every pixel value in a register of its own
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const f32x4 wv = *reinterpret_cast<const f32x4*>(w27 + (ci * 9 + ky * 3 + kx) * E + e);
#pragma unroll
                for (int q = 0; q < SL; ++q) acc[q] += v[q + kx] * wv;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < SL; ++q) {
        if (xs + q >= W) break;
        f32x4 a = acc[q];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = a[i] >= 0.f ? a[i] : 0.01f * a[i];
        *reinterpret_cast<f32x4*>(out + (size_t)((b * H + yh) * W + xs + q) * ld_o + e) = a;
    }
}

// ---------------------------------------------------------------------------------------
// a14: OutputProj conv3x3(C2->CO) (+ global residual), token rows -> NCHW image (model.py:869-890, :1305).
// LPP = C2/4 lanes share a column strip of OP_R vertically adjacent pixels, each lane owning 4 input
// channels; per kx the 3 CO weight vectors (3 ky x CO outputs) are loaded once and the OP_R + 2 token rows of
// the strip feed 3 taps each: at CO = 3, 45 loads per 432 dot-FMAs instead of 36 per 108.  DPP all-reduce over the
// LPP lanes at the end; lanes 0..CO-1 of the group store one output plane each (LPP >= 4 >= CO).
// CO = in_chans of the model (1..4; 3 for RGB): it sizes the accumulators, the weight vectors per tap, the storing lanes and the
// output's plane stride -- per output plane the sums are the same FMAs in the same order at every CO.
// ---------------------------------------------------------------------------------------
constexpr int OP_R = 4;
// lane `sub` (< CO where it stores) picks its plane by a select chain over named elements: indices past CO - 1 repeat the last plane, so the chain
// folds to CO - 1 selects (a helper taking the row by reference left the sums in scratch)
#define UF_PICK_PLANE(A, SUB, CO) \
    (SUB == 0 ? A[0] : (SUB == 1 ? A[CO > 1 ? 1 : 0] : (SUB == 2 ? A[CO > 2 ? 2 : CO - 1] : A[CO - 1])))
template <int LPP, int CO>
__global__ __launch_bounds__(256) void output_proj_kernel(const float* __restrict__ x, int ld_x, const float* __restrict__ w,
                                                          const float* __restrict__ bias, const float* __restrict__ img,
                                                          float* __restrict__ out, int B, int H, int W, int add_img) {
    constexpr int C2 = LPP * 4;
    // grid: x = (pixel column, channel group) of one strip of OP_R rows, y = strip, z = image
    const unsigned idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int sub = (int)(idx % LPP);
    const bool live = idx / LPP < (unsigned)W;
    const int xw = live ? (int)(idx / LPP) : 0, y0 = blockIdx.y * OP_R, b = blockIdx.z;
    f32x4 acc[OP_R][CO];   // per-lane partial sums stay 4 channels wide (pure FMAs); one horizontal add at the end
#pragma unroll
    for (int r = 0; r < OP_R; ++r)
#pragma unroll
        for (int c = 0; c < CO; ++c) acc[r][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    int ro[OP_R + 2];
    float my[OP_R + 2];
#pragma unroll
    for (int hr = 0; hr < OP_R + 2; ++hr) {
        const int iyr = y0 + hr - 1;
        ro[hr] = (b * H + (iyr < 0 ? 0 : (iyr >= H ? H - 1 : iyr))) * W;
        my[hr] = (iyr >= 0 && iyr < H) ? 1.0f : 0.0f;
    }
    const float* xs = x + sub * 4;
    const float* ws = w + sub * 4;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
        const int ixr = xw + kx - 1;
        const int ix = ixr < 0 ? 0 : (ixr >= W ? W - 1 : ixr);
        const float mxk = (ixr >= 0 && ixr < W) ? 1.0f : 0.0f;
        f32x4 wk[3][CO];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int c = 0; c < CO; ++c) wk[ky][c] = *reinterpret_cast<const f32x4*>(ws + (c * 9 + ky * 3 + kx) * C2);
#pragma unroll
        for (int hr = 0; hr < OP_R + 2; ++hr) {
            // zero padding by a 0/1 factor, loads unconditional from clamped addresses, 32-bit element offsets: the product is UNSIGNED (the
            // launcher admits up to 2^32 - 2 elements; as a signed product it overflowed from 2^31 elements on, which is undefined)
            const f32x4 v = (my[hr] * mxk) * *reinterpret_cast<const f32x4*>(xs + (size_t)((unsigned)(ro[hr] + ix) * (unsigned)ld_x));
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int r = hr - ky;
                if (r < 0 || r >= OP_R) continue;
#pragma unroll
                for (int c = 0; c < CO; ++c) acc[r][c] += v * wk[ky][c];
            }
        }
    }
    float a[OP_R][CO];
#pragma unroll
    for (int r = 0; r < OP_R; ++r)
#pragma unroll
        for (int c = 0; c < CO; ++c) a[r][c] = allreduce<RedSum, LPP>((acc[r][c][0] + acc[r][c][1]) + (acc[r][c][2] + acc[r][c][3]));
    if (live && sub < CO) {
        const float bs = bias[sub];
#pragma unroll
        for (int r = 0; r < OP_R; ++r) {
            if (y0 + r >= H) break;
            const size_t o = ((size_t)b * CO + sub) * H * W + (size_t)(y0 + r) * W + xw;
            float v = UF_PICK_PLANE(a[r], sub, CO) + bs;
            if (add_img) v += img[o];  // return x + y (model.py:1305)
            out[o] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------
// a14, second form (round 4): the same convolution with the (4 + 2) x (TW + 2) halo tile of token rows staged in LDS by LDS-DMA.  In the
// first form the three column taps of a pixel are loaded by three different lane groups and the six rows of a strip feed four output rows:
// every token row travels L2 -> L1 -> registers 4.5 times, and the kernel ran at 1.6-2.0 TB/s of its 268 MB input (168 us at 16 x 256 x 256).
// Here a workgroup fetches its tile once (`buffer_load_dwordx4 ... lds`, zero padding = out-of-range buffer offsets), workgroups follow
// the XCD-aware tile order of leff2 (neighbouring tiles share halo rows in one XCD's L2), and the products run from LDS: same
// per-lane partial sums, the same DPP all-reduce, the same order of additions as the first form -- bit-identical results.
// ---------------------------------------------------------------------------------------
template <int LPP, int CO>
__global__ __launch_bounds__(256) void output_proj2_kernel(const float* __restrict__ x, int ld_x, const float* __restrict__ w, const float* __restrict__ bias,
                                                           const float* __restrict__ img, float* __restrict__ out, int B, int H, int W, int add_img, int tiles_x, int tiles_y) {
    constexpr int C2 = LPP * 4, NCOL = 256 / LPP, NX = 2, TW = NX * NCOL, HW2 = TW + 2;
    extern __shared__ __attribute__((aligned(1024))) char smem_op[];
    float* tile = reinterpret_cast<float*>(smem_op);                 // [6][TW + 2][C2]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bt = xcd_tile(blockIdx.x, gridDim.x);
    const int b = bt / (tiles_x * tiles_y), tr = bt - b * (tiles_x * tiles_y);
    const int y0 = (tr / tiles_x) * OP_R, x0 = (tr % tiles_x) * TW;
    {
        const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem_op;
        const unsigned long long xa = (unsigned long long)(uintptr_t)x;
        const u32x4 rsrc = {(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)xa), (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(xa >> 32)) & 0xffffu,
                            (unsigned)__builtin_amdgcn_readfirstlane((int)((unsigned)B * (unsigned)H * (unsigned)W * (unsigned)ld_x * 4u)), 0x00020000u};
        constexpr int NPC = 6 * HW2 * LPP, NINS = (NPC + 63) / 64;
#pragma unroll 1
        for (int idx = wave; idx < NINS; idx += 4) {
            const int q = idx * 64 + lane, hp = q / LPP, part = q - hp * LPP;
            const int r = hp / HW2, c = hp - r * HW2;
            const int iy = y0 - 1 + r, ix = x0 - 1 + c;
            unsigned voff = 0xffffff00u;
            if (hp < 6 * HW2 && iy >= 0 && iy < H && ix >= 0 && ix < W) voff = ((unsigned)((b * H + iy) * W + ix) * (unsigned)ld_x + (unsigned)part * 4u) * 4u;
            dma_buffer_to_lds(rsrc, voff, 0u, lds0 + (unsigned)idx * 1024u);
        }
        wait_dma<0>();
    }
    __syncthreads();
    const int sub = tid % LPP, col = tid / LPP;
    const float* ws = w + sub * 4;
    const float bs = bias[sub < CO ? sub : 0];
#pragma unroll 1
    for (int j = 0; j < NX; ++j) {
        f32x4 acc[OP_R][CO];
#pragma unroll
        for (int r = 0; r < OP_R; ++r)
#pragma unroll
            for (int c = 0; c < CO; ++c) acc[r][c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int kx = 0; kx < 3; ++kx) {                   // not unrolled: nine weight vectors live at a time (the compiler otherwise hoists all 27 out of the column loop)
            f32x4 wk[3][CO];
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int c = 0; c < CO; ++c) wk[ky][c] = *reinterpret_cast<const f32x4*>(ws + (c * 9 + ky * 3 + kx) * C2);
#pragma unroll
            for (int hr = 0; hr < OP_R + 2; ++hr) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(tile + ((hr * HW2) + col + NCOL * j + kx) * C2 + sub * 4);
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) {
                    const int r = hr - ky;
                    if (r < 0 || r >= OP_R) continue;
#pragma unroll
                    for (int c = 0; c < CO; ++c) acc[r][c] += v * wk[ky][c];
                }
            }
        }
        float a[OP_R][CO];
#pragma unroll
        for (int r = 0; r < OP_R; ++r)
#pragma unroll
            for (int c = 0; c < CO; ++c) a[r][c] = allreduce<RedSum, LPP>((acc[r][c][0] + acc[r][c][1]) + (acc[r][c][2] + acc[r][c][3]));
        const int xw = x0 + col + NCOL * j;
        if (sub < CO && xw < W) {
#pragma unroll
            for (int r = 0; r < OP_R; ++r) {
                if (y0 + r >= H) break;
                const size_t o = ((size_t)b * CO + sub) * H * W + (size_t)(y0 + r) * W + xw;
                float v = UF_PICK_PLANE(a[r], sub, CO) + bs;
                if (add_img) v += img[o];
                out[o] = v;
            }
        }
    }
}

// fragment-major weight packing: out[((ntile*KS + kstep)*64 + fg*16 + fr)*8 + e] = W[ntile*16+fr][kstep*32+fg*8+e]
template <typename E>
__global__ void pack_fm_kernel(const E* __restrict__ w, E* __restrict__ out, int N, int K, int KS) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // one 8-element group
    if (idx >= (long long)(N / 16) * KS * 64) return;
    const int lane = (int)(idx & 63), fr = lane & 15, fg = lane >> 4;
    const long long blk = idx >> 6;
    const int ks = (int)(blk % KS), nt = (int)(blk / KS);
    const int n = nt * 16 + fr, k0 = ks * 32 + fg * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) out[idx * 8 + e] = (k0 + e < K) ? w[(size_t)n * K + k0 + e] : E(0);
}

// the way back (K a multiple of 32): w[n][k0 .. k0+7] = one 8-element group of the fragment-major pack
template <typename E>
__global__ void unpack_fm_kernel(const E* __restrict__ fm, E* __restrict__ w, int N, int K, int KS) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // one 8-element group
    if (idx >= (long long)(N / 16) * KS * 64) return;
    const int lane = (int)(idx & 63), fr = lane & 15, fg = lane >> 4;
    const long long blk = idx >> 6;
    const int ks = (int)(blk % KS), nt = (int)(blk / KS);
    const int n = nt * 16 + fr, k0 = ks * 32 + fg * 8;
#pragma unroll
    for (int e = 0; e < 8; ++e) w[(size_t)n * K + k0 + e] = fm[idx * 8 + e];
}

}  // namespace

// fragment-major pack -> row-major T[N][K] (N % 16 == 0, K % 32 == 0): the blocks too wide for the kernels that stream the pack
// (C = 1024) hand their weights to the row-major GEMM this way (uf_model.hip)
int launch_unpack_weight_fm(const void* fm, void* w, int N, int K, uf_dtype dtype, hipStream_t st) {
    UF_REQUIRE(fm && w, UF_ERR_NULL, "unpack_weight_fm: null pointer");
    UF_REQUIRE(N > 0 && K > 0 && N % 16 == 0 && K % 32 == 0, UF_ERR_SHAPE, "unpack_weight_fm: N=%d (multiple of 16) K=%d (multiple of 32)", N, K);
    const int KS = K / 32;
    const long long groups = (long long)(N / 16) * KS * 64;
    dim3 grid((unsigned)((groups + 255) / 256));
    if (dtype_half(dtype)) hipLaunchKernelGGL(unpack_fm_kernel<uint16_t>, grid, dim3(256), 0, st, (const uint16_t*)fm, (uint16_t*)w, N, K, KS);
    else hipLaunchKernelGGL(unpack_fm_kernel<uint32_t>, grid, dim3(256), 0, st, (const uint32_t*)fm, (uint32_t*)w, N, K, KS);
    return check_launch("unpack_weight_fm");
}

int launch_layernorm(const float* x, int ld_x, const float* gamma, const float* beta, const float* modulator, void* out,
                     int rows, int H, int W, int C, int windowed, int shift, uf_dtype dtype, hipStream_t st) {
    char tname[64] = "";
    if (timing_enabled()) snprintf(tname, sizeof(tname), "%s %dx%d", windowed ? "layernorm_window" : "layernorm", rows, C);
    ScopedTimer tm(tname, 8.0 * rows * C, (double)rows * C * (4 + dtype_size(dtype)), st);
#define UF_LN_CASE(CV)                                                                                                  \
    case CV: {                                                                                                          \
        constexpr int LPR = (CV / 4) < 64 ? (CV / 4) : 64;                                                              \
        constexpr int RPB = 256 / LPR;                                                                                  \
        dim3 grid((rows + RPB - 1) / RPB);                                                                              \
        UF_DISPATCH(dtype, TT, hipLaunchKernelGGL((layernorm_kernel<TT, CV>), grid, dim3(256), 0, st, x, ld_x, gamma, beta, modulator, \
                                                  (TT*)out, rows, H, W, windowed, shift));                               \
        break;                                                                                                          \
    }
    switch (C) {
        UF_LN_CASE(16)
        UF_LN_CASE(32)
        UF_LN_CASE(64)
        UF_LN_CASE(128)
        UF_LN_CASE(256)
        UF_LN_CASE(512)
        UF_LN_CASE(1024)
        default:
            set_error("layernorm: C=%d unsupported (16,32,64,128,256,512,1024)", C);
            return UF_ERR_UNSUPPORTED;
    }
#undef UF_LN_CASE
    return check_launch("layernorm");
}

}  // namespace uf

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
using namespace uf;

static int window_copy(const void* src, void* dst, int B, int H, int W, int C, int shift, int elem_bytes, bool reverse,
                       void* stream) {
    UF_REQUIRE(src && dst, UF_ERR_NULL, "window op: null pointer");
    UF_REQUIRE(B > 0 && C > 0 && H % 8 == 0 && W % 8 == 0 && H >= 8 && W >= 8, UF_ERR_SHAPE, "window op: B=%d H=%d W=%d C=%d", B, H, W, C);
    UF_REQUIRE(shift >= 0 && shift < 8, UF_ERR_SHAPE, "window op: shift=%d", shift);
    UF_REQUIRE(elem_bytes == 2 || elem_bytes == 4, UF_ERR_UNSUPPORTED, "window op: elem_bytes=%d (2 or 4)", elem_bytes);
    const int rows = B * H * W;
    hipStream_t st = (hipStream_t)stream;
    const size_t row_bytes = (size_t)C * elem_bytes;
    if (row_bytes % 16 == 0 && ((uintptr_t)src % 16) == 0 && ((uintptr_t)dst % 16) == 0) {
        const int cpr = (int)(row_bytes / 16);
        const long long n = (long long)rows * cpr;
        dim3 grid((unsigned)((n + 255) / 256));
        if (reverse) hipLaunchKernelGGL(window_copy_kernel<true>, grid, dim3(256), 0, st, (const u32x4*)src, (u32x4*)dst, rows, cpr, H, W, shift);
        else hipLaunchKernelGGL(window_copy_kernel<false>, grid, dim3(256), 0, st, (const u32x4*)src, (u32x4*)dst, rows, cpr, H, W, shift);
    } else {
        const long long n = (long long)rows * C;
        dim3 grid((unsigned)((n + 255) / 256));
        if (elem_bytes == 4) {
            if (reverse) hipLaunchKernelGGL((window_copy_elem_kernel<true, uint32_t>), grid, dim3(256), 0, st, (const uint32_t*)src, (uint32_t*)dst, rows, C, H, W, shift);
            else hipLaunchKernelGGL((window_copy_elem_kernel<false, uint32_t>), grid, dim3(256), 0, st, (const uint32_t*)src, (uint32_t*)dst, rows, C, H, W, shift);
        } else {
            if (reverse) hipLaunchKernelGGL((window_copy_elem_kernel<true, uint16_t>), grid, dim3(256), 0, st, (const uint16_t*)src, (uint16_t*)dst, rows, C, H, W, shift);
            else hipLaunchKernelGGL((window_copy_elem_kernel<false, uint16_t>), grid, dim3(256), 0, st, (const uint16_t*)src, (uint16_t*)dst, rows, C, H, W, shift);
        }
    }
    return check_launch("window op");
}

extern "C" size_t uf_weight_fm_elems(int N, int K) { return (N <= 0 || K <= 0 || N % 16) ? 0 : (size_t)N * (size_t)((K + 31) / 32 * 32); }

extern "C" int uf_pack_weight_fm(const void* w, void* out, int N, int K, uf_dtype dtype, void* stream) {
    UF_REQUIRE(w && out, UF_ERR_NULL, "uf_pack_weight_fm: null pointer");
    UF_REQUIRE(N > 0 && K > 0 && N % 16 == 0, UF_ERR_SHAPE, "uf_pack_weight_fm: N=%d must be a positive multiple of 16, K=%d positive", N, K);
    const int KS = (K + 31) / 32;
    const long long groups = (long long)(N / 16) * KS * 64;
    dim3 grid((unsigned)((groups + 255) / 256));
    if (dtype_half(dtype)) hipLaunchKernelGGL(pack_fm_kernel<uint16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const uint16_t*)w, (uint16_t*)out, N, K, KS);
    else if (dtype == UF_F32) hipLaunchKernelGGL(pack_fm_kernel<uint32_t>, grid, dim3(256), 0, (hipStream_t)stream, (const uint32_t*)w, (uint32_t*)out, N, K, KS);
    else { set_error("uf_pack_weight_fm: dtype %d", (int)dtype); return UF_ERR_UNSUPPORTED; }
    return check_launch("pack_weight_fm");
}

extern "C" int uf_window_partition(const void* x, void* out, int B, int H, int W, int C, int shift, int elem_bytes, void* stream) {
    return window_copy(x, out, B, H, W, C, shift, elem_bytes, false, stream);
}
extern "C" int uf_window_reverse(const void* windows, void* out, int B, int H, int W, int C, int shift, int elem_bytes, void* stream) {
    return window_copy(windows, out, B, H, W, C, shift, elem_bytes, true, stream);
}

extern "C" int uf_layernorm_fwd(const float* x, int ld_x, const float* gamma, const float* beta, const float* modulator,
                                void* out, int B, int H, int W, int C, int windowed, int shift, uf_dtype dtype, void* stream) {
    UF_REQUIRE(x && gamma && beta && out, UF_ERR_NULL, "uf_layernorm_fwd: null pointer");
    UF_REQUIRE(B > 0 && H > 0 && W > 0, UF_ERR_SHAPE, "uf_layernorm_fwd: B=%d H=%d W=%d", B, H, W);
    UF_REQUIRE(!windowed || (H % 8 == 0 && W % 8 == 0), UF_ERR_SHAPE, "uf_layernorm_fwd: windowed needs H,W multiples of 8");
    UF_REQUIRE(ld_x >= C && ld_x % 4 == 0, UF_ERR_ALIGN, "uf_layernorm_fwd: ld_x=%d", ld_x);
    UF_REQUIRE(dtype_ok(dtype), UF_ERR_UNSUPPORTED, "uf_layernorm_fwd: dtype %d", (int)dtype);
    return launch_layernorm(x, ld_x, gamma, beta, modulator, out, B * H * W, H, W, C, windowed, shift, dtype, (hipStream_t)stream);
}

// gelu != 0: depthwise 3x3 + bias + GELU (LeFF forward, model.py:659-660).  gelu == 0: the bare stencil (bias may be
// NULL) -- with the taps flipped (w9[8 - t]) it is the INPUT gradient of the same convolution:
// dh[y,x] = sum_{ky,kx} w[ky,kx] dc[y-ky+1, x-kx+1].
namespace {
template <typename T, int ACT>
void launch_dwconv(const void* x, const float* w9, const float* bias, void* out, void* aux, int B, int H, int W, int C, hipStream_t st) {
    if constexpr (ACT != 3) {     // the walking form: W a multiple of 8, tensor under 4 GiB (32-bit byte offsets)
        if (W % 8 == 0 && C % 4 == 0 && (unsigned long long)B * H * W * C * sizeof(T) < 0xffffffffULL) {
            const int seg = W % 16 == 0 ? 16 : 8;
            const long long n = (long long)B * (H / DW_R) * (W / seg) * (C / 4);
            const dim3 grid((unsigned)((n + 255) / 256));
            if (seg == 16) hipLaunchKernelGGL((dwconv3x3_walk_kernel<T, ACT, 16>), grid, dim3(256), 0, st, (const T*)x, w9, bias, (T*)out, (T*)aux, B, H, W, C);
            else hipLaunchKernelGGL((dwconv3x3_walk_kernel<T, ACT, 8>), grid, dim3(256), 0, st, (const T*)x, w9, bias, (T*)out, (T*)aux, B, H, W, C);
            return;
        }
    }
    constexpr int N = Vec16<T>::N;
    const long long n = (long long)B * (H / DW_R) * W * (C / N);
    hipLaunchKernelGGL((dwconv3x3_gelu_kernel<T, ACT>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const T*)x, w9, bias, (T*)out, (T*)aux, B, H, W, C);
}
// mode: 0 plain, 1 + GELU, 2 pre-activation + GELU (two outputs), 3 * GELU'(aux), 4 = 2 on GELU(x) (x is the pre-activation of the GELU in front)
int dwconv_any(const char* fn, const void* x, const float* w9, const float* bias, void* out, void* aux, int B, int H, int W, int C, int mode, uf_dtype dtype, void* stream) {
    UF_REQUIRE(x && w9 && out && (bias || mode == 0 || mode == 3) && (aux || mode < 2), UF_ERR_NULL, "%s: null pointer", fn);
    UF_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && H % DW_R == 0, UF_ERR_SHAPE, "%s: bad shape (H must be a multiple of %d)", fn, DW_R);
    UF_REQUIRE(dtype_ok(dtype), UF_ERR_UNSUPPORTED, "%s: dtype %d", fn, (int)dtype);
    UF_REQUIRE(C % (dtype_half(dtype) ? 8 : 4) == 0, UF_ERR_SHAPE, "%s: C=%d must be a multiple of %d", fn, C, dtype_half(dtype) ? 8 : 4);
    UF_REQUIRE(((uintptr_t)w9 % 16) == 0 && (!bias || ((uintptr_t)bias % 16) == 0), UF_ERR_ALIGN, "%s: w9 / bias must be 16-byte aligned", fn);
    hipStream_t st = (hipStream_t)stream;
    char tname[64] = "";
    if (timing_enabled()) snprintf(tname, sizeof(tname), "dwconv3x3_m%d %dx%d", mode, B * H * W, C);
    ScopedTimer tm(tname, 18.0 * B * H * W * C, (mode >= 2 ? 3.0 : 2.0) * B * H * W * C * dtype_size(dtype), st);
    UF_DISPATCH(dtype, TT, {
        switch (mode) {
            case 0: launch_dwconv<TT, 0>(x, w9, bias, out, aux, B, H, W, C, st); break;
            case 1: launch_dwconv<TT, 1>(x, w9, bias, out, aux, B, H, W, C, st); break;
            case 2: launch_dwconv<TT, 2>(x, w9, bias, out, aux, B, H, W, C, st); break;
            case 4: launch_dwconv<TT, 4>(x, w9, bias, out, aux, B, H, W, C, st); break;
            default: launch_dwconv<TT, 3>(x, w9, bias, out, aux, B, H, W, C, st); break;
        }
    });
    return check_launch("dwconv3x3");
}
}  // namespace

extern "C" int uf_dwconv3x3_fwd(const void* x, const float* w9, const float* bias, void* out, int B, int H, int W, int C, int gelu,
                                uf_dtype dtype, void* stream) {
    return dwconv_any("uf_dwconv3x3_fwd", x, w9, bias, out, nullptr, B, H, W, C, gelu ? 1 : 0, dtype, stream);
}

// training forms (uformer_amd/train.py): the stencil with its pre-activation AND GELU written in one pass (model.py:672-674), and
// the input-gradient stencil (flipped taps, no bias) times GELU'(pre) of the GELU in front of the convolution (model.py:657-658).
extern "C" int uf_dwconv3x3_pre_gelu_fwd(const void* x, const float* w9, const float* bias, void* pre_out, void* act_out, int B, int H, int W, int C,
                                         uf_dtype dtype, void* stream) {
    return dwconv_any("uf_dwconv3x3_pre_gelu_fwd", x, w9, bias, pre_out, act_out, B, H, W, C, 2, dtype, stream);
}

// uf_dwconv3x3_pre_gelu_fwd on x = GELU(pre_in) with the activation applied as the kernel loads pre_in (rounded to T as a stored activation is:
// bit-identical to uf_dwconv3x3_pre_gelu_fwd on the tensor uf_linear_pre_gelu_fwd wrote) -- linear1 then keeps only its pre-activation, one
// hidden-width tensor less written per block and training step.
extern "C" int uf_dwconv3x3_gelu_in_pre_gelu_fwd(const void* pre_in, const float* w9, const float* bias, void* pre_out, void* act_out, int B, int H, int W, int C,
                                                 uf_dtype dtype, void* stream) {
    return dwconv_any("uf_dwconv3x3_gelu_in_pre_gelu_fwd", pre_in, w9, bias, pre_out, act_out, B, H, W, C, 4, dtype, stream);
}

extern "C" int uf_dwconv3x3_mul_dgelu(const void* dy, const float* w9_flipped, const void* pre, void* out, int B, int H, int W, int C, uf_dtype dtype, void* stream) {
    return dwconv_any("uf_dwconv3x3_mul_dgelu", dy, w9_flipped, nullptr, out, const_cast<void*>(pre), B, H, W, C, 3, dtype, stream);
}

extern "C" int uf_dwconv3x3_gelu_fwd(const void* x, const float* w9, const float* bias, void* out, int B, int H, int W, int C,
                                     uf_dtype dtype, void* stream) {
    UF_REQUIRE(bias, UF_ERR_NULL, "uf_dwconv3x3_gelu_fwd: null pointer");
    return uf_dwconv3x3_fwd(x, w9, bias, out, B, H, W, C, 1, dtype, stream);
}

extern "C" int uf_input_proj_fwd(const float* img, const float* w27, const float* bias, float* out, int ld_o, int B, int Cin,
                                 int H, int W, int E, void* stream) {
    UF_REQUIRE(img && w27 && bias && out, UF_ERR_NULL, "uf_input_proj_fwd: null pointer");
    UF_REQUIRE(B > 0 && Cin > 0 && H > 0 && W > 0 && E % 4 == 0 && ld_o >= E && ld_o % 4 == 0, UF_ERR_SHAPE, "uf_input_proj_fwd: bad shape");
    UF_REQUIRE((long long)B * Cin * H * W < 0x7fffffffLL && (long long)Cin * 9 * E < 0x7fffffffLL, UF_ERR_SHAPE, "uf_input_proj_fwd: image too large for 32-bit indexing");
    UF_REQUIRE(H <= 65535 && B <= 65535, UF_ERR_SHAPE, "uf_input_proj_fwd: H=%d B=%d exceed the launch grid", H, B);
    // pixels per thread of the first form: 4 (81 loads per 432 FMAs) or 8 (117 per 864)
    const int px = IP_PX_DEFAULT;
    const unsigned nx = (unsigned)((W + px - 1) / px) * (unsigned)(E / 4);
    ScopedTimer tm("input_proj", 18.0 * B * H * W * Cin * E, 4.0 * B * H * W * (Cin + E), (hipStream_t)stream);
    // The LDS-staged second form (input_proj2_kernel: 107 -> 44 us at 16 x 256 x 256, bit-identical to the first form) is the default since the
    // packed-f32 operand-select hazard that corrupted it beside MFMA kernels was found and removed (see the kernel comment); UF_VARIANT="stem=1": first form.
    const bool v1 = variant("stem", 2) == 1;
    // Built for the image channel counts the reference's tasks use (1, 2, 3, 4, 6); any other Cin, and E = 64, keep the first form.
    const bool cin2 = Cin == 1 || Cin == 2 || Cin == 3 || Cin == 4 || Cin == 6;
    if (!v1 && cin2 && (E == 32 || E == 16) && (H + 3) / 4 <= 65535) {
        const dim3 g32((W + 63) / 64, (H + 3) / 4, B), g16((W + 127) / 128, (H + 3) / 4, B);
#define UF_IP2(CINV)                                                                                                                                     \
        case CINV:                                                                                                                                       \
            if (E == 32) hipLaunchKernelGGL((input_proj2_kernel<8, CINV>), g32, dim3(256), 0, (hipStream_t)stream, img, w27, bias, out, ld_o, B, H, W); \
            else hipLaunchKernelGGL((input_proj2_kernel<4, CINV>), g16, dim3(256), 0, (hipStream_t)stream, img, w27, bias, out, ld_o, B, H, W);         \
            break;
        switch (Cin) {
            UF_IP2(1)
            UF_IP2(2)
            UF_IP2(3)
            UF_IP2(4)
            default: UF_IP2(6)
        }
#undef UF_IP2
        return check_launch("input_proj");
    }
    if (px == 8) hipLaunchKernelGGL(input_proj_kernel<8>, dim3((nx + 255) / 256, H, B), dim3(256), 0, (hipStream_t)stream, img, w27, bias, out, ld_o, B, Cin, H, W, E);
    else hipLaunchKernelGGL(input_proj_kernel<4>, dim3((nx + 255) / 256, H, B), dim3(256), 0, (hipStream_t)stream, img, w27, bias, out, ld_o, B, Cin, H, W, E);
    return check_launch("input_proj");
}

// Cout output planes (1..4).  uf_output_proj_fwd below is the Cout = 3 case.
extern "C" int uf_output_proj_c_fwd(const float* x, int ld_x, const float* w, const float* bias, const float* img, float* out,
                                    int B, int H, int W, int C2, int Cout, int add_img, void* stream) {
    UF_REQUIRE(x && w && bias && out && (!add_img || img), UF_ERR_NULL, "uf_output_proj_fwd: null pointer");
    UF_REQUIRE(B > 0 && H > 0 && W > 0 && ld_x >= C2 && ld_x % 4 == 0, UF_ERR_SHAPE, "uf_output_proj_fwd: bad shape");
    UF_REQUIRE(Cout >= 1 && Cout <= 4, UF_ERR_UNSUPPORTED, "uf_output_proj_fwd: Cout=%d unsupported (1..4)", Cout);
    UF_REQUIRE((long long)B * H * W * ld_x < 0xffffffffLL && H / OP_R < 65535 && B <= 65535, UF_ERR_SHAPE, "uf_output_proj_fwd: tensor too large for 32-bit indexing");
    hipStream_t st = (hipStream_t)stream;
    const long long pix = (long long)B * H * W;
    ScopedTimer tm("output_proj", 18.0 * Cout * pix * C2, 4.0 * pix * (C2 + 2 * Cout), st);
    // one switch over the plane count around every launch: each (LPP, CO) pair is its own kernel
#define UF_OP_CO(LAUNCH)                                                    \
    switch (Cout) {                                                         \
        case 1: LAUNCH(1) break;                                            \
        case 2: LAUNCH(2) break;                                            \
        case 3: LAUNCH(3) break;                                            \
        default: LAUNCH(4) break;                                           \
    }
    {   // second form (LDS-DMA staged halo tile) where the tile fits LDS and 32-bit byte offsets address the tensor; UF_VARIANT="head=1": first form
        const bool v1 = variant("head", 2) == 1;
        if (!v1 && (C2 == 16 || C2 == 32 || C2 == 64) && (long long)B * H * W * ld_x * 4 < 0xffffff00LL) {
            const int lpp = C2 / 4, tw = 2 * (256 / lpp), tiles_x = (W + tw - 1) / tw, tiles_y = (H + OP_R - 1) / OP_R;
            const int smem = (6 * (tw + 2) * C2 * 4 + 1023) / 1024 * 1024;      // whole DMA instructions (1 KiB each): the last one may run past the tile
            const long long nt = (long long)tiles_x * tiles_y * B;
            if (nt < 0x7fffffffLL) {
#define UF_OP2(LPPV, COV)                                                                                                                             \
                {                                                                                                                                     \
                    auto kern = output_proj2_kernel<LPPV, COV>;                                                                                       \
                    static bool lds_done[64] = {};                                                                                                    \
                    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), smem, lds_done, "output_proj")) return rc;                  \
                    hipLaunchKernelGGL(kern, dim3((unsigned)nt), dim3(256), smem, st, x, ld_x, w, bias, img, out, B, H, W, add_img, tiles_x, tiles_y); \
                }
#define UF_OP2_4(COV) UF_OP2(4, COV)
#define UF_OP2_8(COV) UF_OP2(8, COV)
#define UF_OP2_16(COV) UF_OP2(16, COV)
                if (lpp == 4) { UF_OP_CO(UF_OP2_4) } else if (lpp == 8) { UF_OP_CO(UF_OP2_8) } else { UF_OP_CO(UF_OP2_16) }
#undef UF_OP2_4
#undef UF_OP2_8
#undef UF_OP2_16
#undef UF_OP2
                return check_launch("output_proj");
            }
        }
    }
#define UF_OP1(LPPV, COV)                                                                                                               \
    {                                                                                                                                   \
        const unsigned nx = (unsigned)W * LPPV;                                                                                         \
        hipLaunchKernelGGL((output_proj_kernel<LPPV, COV>), dim3((nx + 255) / 256, (H + OP_R - 1) / OP_R, B), dim3(256), 0, st, x, ld_x, \
                           w, bias, img, out, B, H, W, add_img);                                                                        \
    }
#define UF_OP1_4(COV) UF_OP1(4, COV)
#define UF_OP1_8(COV) UF_OP1(8, COV)
#define UF_OP1_16(COV) UF_OP1(16, COV)
#define UF_OP1_32(COV) UF_OP1(32, COV)
    switch (C2) {
        case 16: UF_OP_CO(UF_OP1_4) break;
        case 32: UF_OP_CO(UF_OP1_8) break;
        case 64: UF_OP_CO(UF_OP1_16) break;
        case 128: UF_OP_CO(UF_OP1_32) break;
        default:
            set_error("uf_output_proj_fwd: C2=%d unsupported (16,32,64,128)", C2);
            return UF_ERR_UNSUPPORTED;
    }
#undef UF_OP1_4
#undef UF_OP1_8
#undef UF_OP1_16
#undef UF_OP1_32
#undef UF_OP1
#undef UF_OP_CO
    return check_launch("output_proj");
}

extern "C" int uf_output_proj_fwd(const float* x, int ld_x, const float* w, const float* bias, const float* img, float* out,
                                  int B, int H, int W, int C2, int add_img, void* stream) {
    return uf_output_proj_c_fwd(x, ld_x, w, bias, img, out, B, H, W, C2, 3, add_img, stream);
}
