// 4x4-window LeWin blocks: the bottleneck of a Uformer built for 64x64 patches (img_size 64: the stage's resolution is 4, so
// LeWinTransformerBlock clamps its window to 4 and its shift to 0, model.py:863-866).  Window attention forward and backward over
// 16-token windows, the gradient of the 7x7 relative-position table, window partition / reverse at 4, the block forward and the
// whole-model entry's bottleneck.
//
// The window geometry is folded into the kernels' addressing: q|k|v, the attention output and every gradient stay in raster token
// order (B*H*W rows), so the token-wise ops of the block (LayerNorm, projections, LeFF) run on raster rows with no partition pass.
// One workgroup = one window x W4_NH heads, one lane per (head, query row); the 16 key rows of q, k, v (and dO) are staged in LDS as
// f32.  Scores, softmax and both products accumulate in f32 from the stored operand type T (the same rounding points as the 8x8
// path: q, k, v and o are T).  The work is tiny (a 16x16 tile per head), so the kernels are latency- not throughput-bound; they
// use the vector ALUs rather than MFMA (DESIGN.md "4x4-window bottleneck").
#include <math.h>

#include "uf_internal.h"

namespace uf {

int launch_layernorm(const float* x, int ld_x, const float* gamma, const float* beta, const float* modulator, void* out,
                     int rows, int H, int W, int C, int windowed, int shift, uf_dtype dtype, hipStream_t st);

namespace {

constexpr int W4_NH = 4;                 // heads per workgroup
constexpr int W4_THREADS = 16 * W4_NH;   // one wave: lane = head_local * 16 + query row

template <typename T> struct W4Vec { static constexpr int N = 8; };   // elements per 16-byte access
template <> struct W4Vec<float> { static constexpr int N = 4; };

template <typename T> __device__ __forceinline__ void w4_load(const T* p, float* f) {
    if constexpr (std::is_same<T, float>::value) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p);
        f[0] = v[0]; f[1] = v[1]; f[2] = v[2]; f[3] = v[3];
    } else {
        unpack8<T>(*reinterpret_cast<const u32x4*>(p), f);
    }
}

template <typename T> __device__ __forceinline__ void w4_store(T* p, const float* f) {
    if constexpr (std::is_same<T, float>::value) *reinterpret_cast<f32x4*>(p) = f32x4{f[0], f[1], f[2], f[3]};
    else *reinterpret_cast<u32x4*>(p) = pack8<T>(f);
}

// raster row of token t (0..15, row-major inside the window) of window `win` (windows image-major, then row-major: window_partition's order)
__device__ __forceinline__ int w4_row(int win, int t, int H, int W) {
    const int nwx = W >> 2, per_img = (H >> 2) * nwx;
    const int b = win / per_img, r = win - b * per_img;
    const int wy = r / nwx, wx = r - wy * nwx;
    return (b * H + wy * 4 + (t >> 2)) * W + wx * 4 + (t & 3);
}

// LDS row stride of the staged operands: 4 floats of padding keeps rows 16-byte aligned and puts row i on bank 4 i
template <int HD> constexpr int w4_ls() { return W4_NH * HD + 4; }

// stage columns [col0, col0 + ncols) of the 16 rows of window `win` into dst[16][LS] as f32
template <typename T, int LS>
__device__ __forceinline__ void w4_stage(float* dst, const T* __restrict__ src, int ld, int col0, int ncols, int win, int H, int W) {
    constexpr int V = W4Vec<T>::N;
    const int per_row = ncols / V;
    for (int e = threadIdx.x; e < 16 * per_row; e += W4_THREADS) {
        const int t = e / per_row, c = (e - t * per_row) * V;
        float f[V];
        w4_load<T>(src + (size_t)w4_row(win, t, H, W) * ld + col0 + c, f);
#pragma unroll
        for (int v = 0; v < V; ++v) dst[t * LS + c + v] = f[v];
    }
}

// bias of (query i, key j) from the (heads, 49) table: entry (yi - yj + 3) * 7 + (xi - xj + 3)   (model.py:467-477, 500-502)
__device__ __forceinline__ int w4_entry(int i, int j) { return ((i >> 2) - (j >> 2) + 3) * 7 + ((i & 3) - (j & 3) + 3); }

// scores of query row i against the 16 keys, softmax in place: p[j]
template <int HD, int LS>
__device__ __forceinline__ void w4_softmax_row(const float* q, const float* sk, int hl, int i, const float* __restrict__ tab, float scale, float* p) {
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const float* kr = sk + j * LS + hl * HD;
        float acc = 0.f;
#pragma unroll
        for (int d = 0; d < HD; ++d) acc = fmaf(q[d], kr[d], acc);
        p[j] = acc * scale + tab[w4_entry(i, j)];
        m = fmaxf(m, p[j]);
    }
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        p[j] = expf(p[j] - m);
        sum += p[j];
    }
    const float inv = 1.f / sum;
#pragma unroll
    for (int j = 0; j < 16; ++j) p[j] *= inv;
}

template <typename T, int HD>
__global__ __launch_bounds__(W4_THREADS) void win4_attn_fwd_kernel(const T* __restrict__ qkv, int ld, const float* __restrict__ rpb4, T* __restrict__ o,
                                                                  int ldo, int H, int W, int C, int heads, int n_groups, float scale) {
    constexpr int LS = w4_ls<HD>(), V = W4Vec<T>::N;
    __shared__ __attribute__((aligned(16))) float sq[16 * LS];
    __shared__ __attribute__((aligned(16))) float sk[16 * LS];
    __shared__ __attribute__((aligned(16))) float sv[16 * LS];
    const int win = blockIdx.x / n_groups, h0 = (blockIdx.x - win * n_groups) * W4_NH;
    const int nh = heads - h0 < W4_NH ? heads - h0 : W4_NH;
    w4_stage<T, LS>(sq, qkv, ld, h0 * HD, nh * HD, win, H, W);
    w4_stage<T, LS>(sk, qkv, ld, C + h0 * HD, nh * HD, win, H, W);
    w4_stage<T, LS>(sv, qkv, ld, 2 * C + h0 * HD, nh * HD, win, H, W);
    __syncthreads();
    const int hl = threadIdx.x >> 4, i = threadIdx.x & 15;
    if (hl >= nh) return;
    const int h = h0 + hl;
    float q[HD], p[16], acc[HD];
#pragma unroll
    for (int d = 0; d < HD; ++d) q[d] = sq[i * LS + hl * HD + d];
    w4_softmax_row<HD, LS>(q, sk, hl, i, rpb4 + h * 49, scale, p);
#pragma unroll
    for (int d = 0; d < HD; ++d) acc[d] = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const float* vr = sv + j * LS + hl * HD;
#pragma unroll
        for (int d = 0; d < HD; ++d) acc[d] = fmaf(p[j], vr[d], acc[d]);
    }
    T* orow = o + (size_t)w4_row(win, i, H, W) * ldo + h * HD;
#pragma unroll
    for (int d = 0; d < HD; d += V) w4_store<T>(orow + d, acc + d);
}

// dS = P (dP - rowsum(P dP)), dP = dO V^T; dq = scale dS K, dk = scale dS^T q, dv = P^T dO.  dscore (f32, (n_windows, heads, 16, 16))
// keeps dS per window for the table gradient (a fixed-order sum, uf_rpb4_table_grad: no float atomics).
template <typename T, int HD>
__global__ __launch_bounds__(W4_THREADS) void win4_attn_bwd_kernel(const T* __restrict__ qkv, int ld, const float* __restrict__ rpb4, const T* __restrict__ dout,
                                                                  int ld_do, T* __restrict__ dqkv, int ld_dq, float* __restrict__ dscore, int H, int W, int C,
                                                                  int heads, int n_groups, float scale) {
    constexpr int LS = w4_ls<HD>(), V = W4Vec<T>::N;
    __shared__ __attribute__((aligned(16))) float sq[16 * LS];
    __shared__ __attribute__((aligned(16))) float sk[16 * LS];
    __shared__ __attribute__((aligned(16))) float sv[16 * LS];
    __shared__ __attribute__((aligned(16))) float sdo[16 * LS];
    __shared__ float sp[W4_NH][16][17];
    __shared__ float sds[W4_NH][16][17];
    const int win = blockIdx.x / n_groups, h0 = (blockIdx.x - win * n_groups) * W4_NH;
    const int nh = heads - h0 < W4_NH ? heads - h0 : W4_NH;
    w4_stage<T, LS>(sq, qkv, ld, h0 * HD, nh * HD, win, H, W);
    w4_stage<T, LS>(sk, qkv, ld, C + h0 * HD, nh * HD, win, H, W);
    w4_stage<T, LS>(sv, qkv, ld, 2 * C + h0 * HD, nh * HD, win, H, W);
    w4_stage<T, LS>(sdo, dout, ld_do, h0 * HD, nh * HD, win, H, W);
    __syncthreads();
    const int hl = threadIdx.x >> 4, i = threadIdx.x & 15;
    const bool active = hl < nh;
    const int h = h0 + hl;
    if (active) {                                        // query role: row i of dS, dq_i
        float q[HD], p[16], g[HD];
#pragma unroll
        for (int d = 0; d < HD; ++d) q[d] = sq[i * LS + hl * HD + d];
        w4_softmax_row<HD, LS>(q, sk, hl, i, rpb4 + h * 49, scale, p);
#pragma unroll
        for (int d = 0; d < HD; ++d) g[d] = sdo[i * LS + hl * HD + d];
        float dp[16], rs = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float* vr = sv + j * LS + hl * HD;
            float acc = 0.f;
#pragma unroll
            for (int d = 0; d < HD; ++d) acc = fmaf(g[d], vr[d], acc);
            dp[j] = acc;
            rs = fmaf(p[j], acc, rs);
        }
        float* ds_out = dscore + ((size_t)win * heads + h) * 256 + i * 16;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float ds = p[j] * (dp[j] - rs);
            sp[hl][i][j] = p[j];
            sds[hl][i][j] = ds;
            ds_out[j] = ds;
        }
#pragma unroll
        for (int d = 0; d < HD; ++d) g[d] = 0.f;
        // dS row read back from LDS (this lane's own stores): a rolled loop keeps the registers of the 16 x HD products bounded
#pragma unroll 2
        for (int j = 0; j < 16; ++j) {
            const float ds = sds[hl][i][j];
            const float* kr = sk + j * LS + hl * HD;
#pragma unroll
            for (int d = 0; d < HD; ++d) g[d] = fmaf(ds, kr[d], g[d]);
        }
#pragma unroll
        for (int d = 0; d < HD; ++d) g[d] *= scale;
        T* dq = dqkv + (size_t)w4_row(win, i, H, W) * ld_dq + h * HD;
#pragma unroll
        for (int d = 0; d < HD; d += V) w4_store<T>(dq + d, g + d);
    }
    __syncthreads();
    if (!active) return;
    const int j = i;                                     // key role: dk_j, dv_j
    float dk[HD], dv[HD];
#pragma unroll
    for (int d = 0; d < HD; ++d) { dk[d] = 0.f; dv[d] = 0.f; }
#pragma unroll 2
    for (int r = 0; r < 16; ++r) {
        const float ds = sds[hl][r][j], pr = sp[hl][r][j];
        const float* qr = sq + r * LS + hl * HD;
        const float* gr = sdo + r * LS + hl * HD;
#pragma unroll
        for (int d = 0; d < HD; ++d) {
            dk[d] = fmaf(ds, qr[d], dk[d]);
            dv[d] = fmaf(pr, gr[d], dv[d]);
        }
    }
#pragma unroll
    for (int d = 0; d < HD; ++d) dk[d] *= scale;
    T* row = dqkv + (size_t)w4_row(win, j, H, W) * ld_dq;
#pragma unroll
    for (int d = 0; d < HD; d += V) {
        w4_store<T>(row + C + h * HD + d, dk + d);
        w4_store<T>(row + 2 * C + h * HD + d, dv + d);
    }
}

// (49, heads) table gradient: per head, dS summed over the windows (four interleaved partial sums, added in a fixed order), then
// every entry gathers its (query, key) pairs in row-major order.  Deterministic.
__global__ __launch_bounds__(1024) void rpb4_table_grad_kernel(const float* __restrict__ dscore, float* __restrict__ dtable, int n_windows, int heads) {
    __shared__ float part[4][256];
    const int h = blockIdx.x, e = threadIdx.x & 255, lane = threadIdx.x >> 8;
    float acc = 0.f;
    for (int w = lane; w < n_windows; w += 4) acc += dscore[((size_t)w * heads + h) * 256 + e];
    part[lane][e] = acc;
    __syncthreads();
    if (threadIdx.x < 256) part[0][e] = ((part[0][e] + part[1][e]) + part[2][e]) + part[3][e];
    __syncthreads();
    if (threadIdx.x < 49) {
        const int dy = (int)threadIdx.x / 7 - 3, dx = (int)threadIdx.x % 7 - 3;
        float s = 0.f;
        for (int i = 0; i < 16; ++i) {
            const int yj = (i >> 2) - dy, xj = (i & 3) - dx;
            if (yj >= 0 && yj < 4 && xj >= 0 && xj < 4) s += part[0][i * 16 + yj * 4 + xj];
        }
        dtable[threadIdx.x * heads + h] = s;
    }
}

// window_partition / window_reverse at 4 (model.py:704-726): element copies between raster rows and window rows
template <bool REV, typename E>
__global__ void win4_copy_kernel(const E* __restrict__ src, E* __restrict__ dst, long long n, int C, int H, int W) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int r = (int)(idx / C), c = (int)(idx - (long long)r * C);
    const long long raster = (long long)w4_row(r >> 4, r & 15, H, W) * C + c;
    if (REV) dst[raster] = src[idx];
    else dst[idx] = src[raster];
}

int check_attn4(const char* fn, int B, int H, int W, int C, int heads, int ld, uf_dtype dtype) {
    UF_REQUIRE(dtype_ok(dtype), UF_ERR_UNSUPPORTED, "%s: dtype %d", fn, (int)dtype);
    UF_REQUIRE(B > 0 && H > 0 && W > 0 && H % 4 == 0 && W % 4 == 0, UF_ERR_SHAPE, "%s: B=%d H=%d W=%d (H, W multiples of 4)", fn, B, H, W);
    UF_REQUIRE(heads > 0 && C % heads == 0, UF_ERR_SHAPE, "%s: C=%d heads=%d", fn, C, heads);
    const int hd = C / heads;
    UF_REQUIRE(hd == 16 || hd == 32, UF_ERR_UNSUPPORTED, "%s: head_dim %d (16 or 32 supported)", fn, hd);
    UF_REQUIRE(ld >= 3 * C && ld % 8 == 0, UF_ERR_ALIGN, "%s: ld_qkv=%d (>= 3C, a multiple of 8)", fn, ld);
    UF_REQUIRE((long long)B * H * W * ld < 0x7fffffffLL, UF_ERR_SHAPE, "%s: tensor too large for 32-bit row indexing", fn);
    return UF_OK;
}

size_t block4_ws_bytes(size_t M, size_t C, uf_dtype dtype) {   // = uf_block_workspace_bytes: T[M][C] + 2 x T[M][4C] (q|k|v fits in the first T[M][4C])
    const size_t sz = dtype_size(dtype);
    return align_up(M * C * sz, 256) + 2 * align_up(M * 4 * C * sz, 256);
}

}  // namespace
}  // namespace uf

using namespace uf;

extern "C" int uf_window4_attention_fwd(const void* qkv, int ld_qkv, const float* rpb4, void* o, int ld_o, int B, int H, int W, int C, int heads,
                                        uf_dtype dtype, void* stream) {
    UF_REQUIRE(qkv && rpb4 && o, UF_ERR_NULL, "uf_window4_attention_fwd: null pointer");
    int rc = check_attn4("uf_window4_attention_fwd", B, H, W, C, heads, ld_qkv, dtype);
    if (rc) return rc;
    UF_REQUIRE(ld_o >= C && ld_o % 8 == 0 && ((uintptr_t)qkv % 16) == 0 && ((uintptr_t)o % 16) == 0, UF_ERR_ALIGN,
               "uf_window4_attention_fwd: ld_o=%d (>= C, a multiple of 8), qkv / o 16-byte aligned", ld_o);
    const int hd = C / heads, n_groups = (heads + W4_NH - 1) / W4_NH, n_windows = B * (H / 4) * (W / 4);
    const float scale = (float)(1.0 / sqrt((double)hd));
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(n_windows * n_groups));
    UF_DISPATCH(dtype, TT, {
        if (hd == 32) hipLaunchKernelGGL((win4_attn_fwd_kernel<TT, 32>), grid, dim3(W4_THREADS), 0, st, (const TT*)qkv, ld_qkv, rpb4, (TT*)o, ld_o, H, W, C, heads, n_groups, scale);
        else hipLaunchKernelGGL((win4_attn_fwd_kernel<TT, 16>), grid, dim3(W4_THREADS), 0, st, (const TT*)qkv, ld_qkv, rpb4, (TT*)o, ld_o, H, W, C, heads, n_groups, scale);
    });
    return check_launch("window4_attention_fwd");
}

extern "C" int uf_window4_attention_bwd(const void* qkv, int ld_qkv, const float* rpb4, const void* dout, int ld_do, void* dqkv, int ld_dqkv,
                                        float* dscore, int B, int H, int W, int C, int heads, uf_dtype dtype, void* stream) {
    UF_REQUIRE(qkv && rpb4 && dout && dqkv && dscore, UF_ERR_NULL, "uf_window4_attention_bwd: null pointer");
    int rc = check_attn4("uf_window4_attention_bwd", B, H, W, C, heads, ld_qkv, dtype);
    if (rc) return rc;
    UF_REQUIRE(ld_do >= C && ld_do % 8 == 0 && ld_dqkv >= 3 * C && ld_dqkv % 8 == 0, UF_ERR_ALIGN, "uf_window4_attention_bwd: ld_do=%d ld_dqkv=%d", ld_do, ld_dqkv);
    UF_REQUIRE(((uintptr_t)qkv % 16) == 0 && ((uintptr_t)dout % 16) == 0 && ((uintptr_t)dqkv % 16) == 0, UF_ERR_ALIGN,
               "uf_window4_attention_bwd: operands must be 16-byte aligned");
    const int hd = C / heads, n_groups = (heads + W4_NH - 1) / W4_NH, n_windows = B * (H / 4) * (W / 4);
    const float scale = (float)(1.0 / sqrt((double)hd));
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(n_windows * n_groups));
    UF_DISPATCH(dtype, TT, {
        if (hd == 32) hipLaunchKernelGGL((win4_attn_bwd_kernel<TT, 32>), grid, dim3(W4_THREADS), 0, st, (const TT*)qkv, ld_qkv, rpb4, (const TT*)dout, ld_do,
                                         (TT*)dqkv, ld_dqkv, dscore, H, W, C, heads, n_groups, scale);
        else hipLaunchKernelGGL((win4_attn_bwd_kernel<TT, 16>), grid, dim3(W4_THREADS), 0, st, (const TT*)qkv, ld_qkv, rpb4, (const TT*)dout, ld_do,
                                (TT*)dqkv, ld_dqkv, dscore, H, W, C, heads, n_groups, scale);
    });
    return check_launch("window4_attention_bwd");
}

extern "C" int uf_rpb4_table_grad(const float* dscore, float* dtable, int n_windows, int heads, void* stream) {
    UF_REQUIRE(dscore && dtable, UF_ERR_NULL, "uf_rpb4_table_grad: null pointer");
    UF_REQUIRE(n_windows > 0 && heads > 0, UF_ERR_SHAPE, "uf_rpb4_table_grad: n_windows=%d heads=%d", n_windows, heads);
    hipLaunchKernelGGL(rpb4_table_grad_kernel, dim3(heads), dim3(1024), 0, (hipStream_t)stream, dscore, dtable, n_windows, heads);
    return check_launch("rpb4_table_grad");
}

static int window4_copy(const void* src, void* dst, int B, int H, int W, int C, int elem_bytes, bool reverse, void* stream) {
    UF_REQUIRE(src && dst, UF_ERR_NULL, "window4 op: null pointer");
    UF_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && H % 4 == 0 && W % 4 == 0, UF_ERR_SHAPE, "window4 op: B=%d H=%d W=%d C=%d", B, H, W, C);
    UF_REQUIRE(elem_bytes == 2 || elem_bytes == 4, UF_ERR_UNSUPPORTED, "window4 op: elem_bytes=%d (2 or 4)", elem_bytes);
    const long long n = (long long)B * H * W * C;
    UF_REQUIRE(n < 0x7fffffffLL * 16LL, UF_ERR_SHAPE, "window4 op: tensor too large");
    const dim3 grid((unsigned)((n + 255) / 256));
    hipStream_t st = (hipStream_t)stream;
    if (elem_bytes == 4) {
        if (reverse) hipLaunchKernelGGL((win4_copy_kernel<true, uint32_t>), grid, dim3(256), 0, st, (const uint32_t*)src, (uint32_t*)dst, n, C, H, W);
        else hipLaunchKernelGGL((win4_copy_kernel<false, uint32_t>), grid, dim3(256), 0, st, (const uint32_t*)src, (uint32_t*)dst, n, C, H, W);
    } else {
        if (reverse) hipLaunchKernelGGL((win4_copy_kernel<true, uint16_t>), grid, dim3(256), 0, st, (const uint16_t*)src, (uint16_t*)dst, n, C, H, W);
        else hipLaunchKernelGGL((win4_copy_kernel<false, uint16_t>), grid, dim3(256), 0, st, (const uint16_t*)src, (uint16_t*)dst, n, C, H, W);
    }
    return check_launch("window4 op");
}

extern "C" int uf_window4_partition(const void* x, void* out, int B, int H, int W, int C, int elem_bytes, void* stream) {
    return window4_copy(x, out, B, H, W, C, elem_bytes, false, stream);
}
extern "C" int uf_window4_reverse(const void* windows, void* out, int B, int H, int W, int C, int elem_bytes, void* stream) {
    return window4_copy(windows, out, B, H, W, C, elem_bytes, true, stream);
}

// LN1 -> q|k|v (raster rows) -> 4x4-window attention -> proj + residual -> LN2 -> linear1 + GELU -> depthwise 3x3 + GELU -> linear2 + residual
// (model.py:951-987 with window 4, shift 0, no modulator).  Workspace: uf_block_workspace_bytes(B*H*W, C, dtype).
extern "C" int uf_lewin_block4_fwd(const uf_block4_params* p, float* x, int ld, int B, int H, int W, int C, const float* drop_attn,
                                   const float* drop_leff, uf_dtype dtype, void* ws, size_t ws_bytes, void* stream) {
    UF_REQUIRE(p && x && ws, UF_ERR_NULL, "uf_lewin_block4_fwd: null pointer");
    UF_REQUIRE(p->wdw9 || p->bdw, UF_ERR_UNSUPPORTED, "uf_lewin_block4_fwd: a block without depthwise weights (token_mlp = 'ffn') is not built for 4x4 windows");
    UF_REQUIRE(p->norm1_w && p->norm1_b && p->norm2_w && p->norm2_b && p->rpb4 && p->wqkv && p->bqkv && p->wproj && p->bproj && p->w1 && p->b1 &&
               p->wdw9 && p->bdw && p->w2 && p->b2, UF_ERR_NULL, "uf_lewin_block4_fwd: null parameter");
    int rc = check_attn4("uf_lewin_block4_fwd", B, H, W, C, p->heads, 3 * C, dtype);
    if (rc) return rc;
    UF_REQUIRE(C % 16 == 0 && ld >= C && ld % 4 == 0 && ((uintptr_t)x % 16) == 0, UF_ERR_SHAPE, "uf_lewin_block4_fwd: C=%d ld=%d", C, ld);
    UF_REQUIRE(((uintptr_t)ws % 256) == 0, UF_ERR_ALIGN, "uf_lewin_block4_fwd: workspace must be 256-byte aligned");
    const size_t M = (size_t)B * H * W, sz = dtype_size(dtype);
    const size_t need = block4_ws_bytes(M, C, dtype);
    UF_REQUIRE(ws_bytes >= need, UF_ERR_WORKSPACE, "uf_lewin_block4_fwd: workspace too small: %zu < %zu bytes", ws_bytes, need);
    char* a = (char*)ws;                              // T[M][C]:  LN output, then the attention output
    char* h1 = a + align_up(M * C * sz, 256);         // T[M][4C]: q|k|v (M x 3C), then the LeFF hidden
    char* h2 = h1 + align_up(M * 4 * C * sz, 256);    // T[M][4C]: the LeFF hidden after the depthwise conv
    hipStream_t st = (hipStream_t)stream;
    rc = launch_layernorm(x, ld, p->norm1_w, p->norm1_b, nullptr, a, (int)M, H, W, C, 0, 0, dtype, st);
    if (rc) return rc;
    GemmParams g{};
    g.A = a; g.lda = C; g.W = p->wqkv; g.bias = p->bqkv; g.M = (int)M; g.N = 3 * C; g.K = C; g.out = h1; g.ldo = 3 * C;
    rc = launch_gemm(g, A_PLAIN, E_STORE_T, dtype, st);
    if (rc) return rc;
    rc = uf_window4_attention_fwd(h1, 3 * C, p->rpb4, a, C, B, H, W, C, p->heads, dtype, stream);
    if (rc) return rc;
    g = GemmParams{};
    g.A = a; g.lda = C; g.W = p->wproj; g.bias = p->bproj; g.M = (int)M; g.N = C; g.K = C;
    g.out = x; g.ldo = ld; g.resid = x; g.ldr = ld; g.scale = drop_attn; g.hw = H * W;
    rc = launch_gemm(g, A_PLAIN, E_RES, dtype, st);
    if (rc) return rc;
    rc = launch_layernorm(x, ld, p->norm2_w, p->norm2_b, nullptr, a, (int)M, H, W, C, 0, 0, dtype, st);
    if (rc) return rc;
    g = GemmParams{};
    g.A = a; g.lda = C; g.W = p->w1; g.bias = p->b1; g.M = (int)M; g.N = 4 * C; g.K = C; g.out = h1; g.ldo = 4 * C;
    rc = launch_gemm(g, A_PLAIN, E_STORE_T_GELU, dtype, st);
    if (rc) return rc;
    rc = uf_dwconv3x3_fwd(h1, p->wdw9, p->bdw, h2, B, H, W, 4 * C, 1, dtype, stream);
    if (rc) return rc;
    g = GemmParams{};
    g.A = h2; g.lda = 4 * C; g.W = p->w2; g.bias = p->b2; g.M = (int)M; g.N = C; g.K = 4 * C;
    g.out = x; g.ldo = ld; g.resid = x; g.ldr = ld; g.scale = drop_leff; g.hw = H * W;
    return launch_gemm(g, A_PLAIN, E_RES, dtype, st);
}
