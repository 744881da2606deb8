// uint8 frames in and out of the model on the device: the conversions either side of infer.restore / infer.restore_tiled as
// four byte-moving kernels, none with matrix work.
//   uf_frames_to_canvas   u8 frames (interleaved or planar) -> zero-padded f32 canvas (+ mask), u / 255 like load_img (utils/image_utils.py:31-35)
//   uf_canvas_to_frames   crop + clamp + quantise: img_as_ubyte(clamp(x, 0, 1)) of test/test_gopro_hide.py:103-110 for float32 input
//   uf_tiles_gather       the tile batch of infer.restore_tiled (torch.cat(tiles, 0)) from u8 or f32 frames
//   uf_tiles_blend        the ramp-weighted sum of the restored tiles over the sum of the weights, as f32 planes or u8 frames
// One workgroup owns one output row segment of SEG columns.  The frame side of a segment is one run of bytes (interleaved) or one run per channel
// (planar): it moves between global memory and LDS as 16-byte accesses over the aligned body of the run and single bytes over the < 16 at each end,
// at the LDS offset that has the global address's low four bits, so that both sides of every 16-byte copy are aligned for any row length and any
// channel count.  The f32 side is read and written four columns per lane (one 16-byte access) when the row pitch and the base pointer allow it.
// The transposition between the two layouts is the LDS access pattern.  The u8 results reach memory as the dwords assembled in LDS.
#include "uf_internal.h"

namespace uf {
namespace {

constexpr int SEG = 1024;               // output columns per workgroup: 256 lanes x 4
constexpr int MAX_C = 8;                // channels on the input side
constexpr int MAX_C_U8 = 4;             // channels of a u8 result
constexpr int MAX_STARTS = 64;          // tile starts per axis of uf_tiles_blend
constexpr long long LIMIT31 = 1LL << 31;

// run of n bytes at g -> LDS region l (16-byte aligned), byte i at l[(g & 15) + i]
__device__ __forceinline__ void run_to_lds(const unsigned char* __restrict__ g, unsigned char* l, int n) {
    const int sh = (int)((uintptr_t)g & 15);
    const int head = sh ? (16 - sh < n ? 16 - sh : n) : 0;
    const int body = (n - head) >> 4;
    const int tail0 = head + body * 16;
    for (int i = threadIdx.x; i < body; i += 256) *reinterpret_cast<u32x4*>(l + sh + head + 16 * i) = *reinterpret_cast<const u32x4*>(g + head + 16 * i);
    if ((int)threadIdx.x < head) l[sh + threadIdx.x] = g[threadIdx.x];
    const int t = tail0 + (int)threadIdx.x - 64;                     // the second wave takes the tail
    if (t >= tail0 && t < n) l[sh + t] = g[t];
}
// the way back: LDS region l (byte i at l[(g & 15) + i]) -> n bytes at g; whole dwords x 4 over the aligned body
__device__ __forceinline__ void lds_to_run(const unsigned char* l, unsigned char* __restrict__ g, int n) {
    const int sh = (int)((uintptr_t)g & 15);
    const int head = sh ? (16 - sh < n ? 16 - sh : n) : 0;
    const int body = (n - head) >> 4;
    const int tail0 = head + body * 16;
    for (int i = threadIdx.x; i < body; i += 256) *reinterpret_cast<u32x4*>(g + head + 16 * i) = *reinterpret_cast<const u32x4*>(l + sh + head + 16 * i);
    if ((int)threadIdx.x < head) g[threadIdx.x] = l[sh + threadIdx.x];
    const int t = tail0 + (int)threadIdx.x - 64;
    if (t >= tail0 && t < n) g[t] = l[sh + t];
}

__device__ __forceinline__ int swapped(int c, int swap_rb) { return swap_rb ? (c == 0 ? 2 : (c == 2 ? 0 : c)) : c; }
__device__ __forceinline__ float to_unit(unsigned char u) { return (float)u / 255.0f; }      // IEEE division, as crop_aug_kernel
__device__ __forceinline__ float to_unit(float v) { return v; }
// img_as_ubyte(clamp(v, 0, 1)) for float32: rint(v * 255) with the product in f32, ties to even; NaN -> 0 (fmaxf returns the other operand)
__device__ __forceinline__ unsigned char quantise(float v) {
    const float q = __builtin_rintf(fminf(fmaxf(v, 0.0f), 1.0f) * 255.0f);
    return (unsigned char)(int)q;
}

// ---- frames -> canvas, frames -> tiles ----------------------------------------------------------------------------------------------
// out (NI,C,OH,OW) f32: image i shows frame i % B with the frame's pixel (0,0) at output (y0,x0), zero where there is no frame; origins
// (device, [NI / B][2] = y, x of the frame pixel at the output's (0,0)) replaces the uniform (y0,x0) by (-y, -x) per group of B images.
// mask (NI,1,OH,OW) or NULL: 1 over the frame.  Every output element is written exactly once.
template <typename S, bool VEC>
__global__ __launch_bounds__(256) void paste_rows_kernel(const S* __restrict__ src, int hwc, int swap_rb, float* __restrict__ out, float* __restrict__ mask,
                                                         const int* __restrict__ origins, int B, int C, int h, int w, int OH, int OW, int y0, int x0, int nseg) {
    constexpr int REG = SEG * (int)sizeof(S) + 16;                   // bytes of LDS per planar channel run
    __shared__ __attribute__((aligned(16))) unsigned char lds[MAX_C * REG];
    const int seg = blockIdx.x % nseg, row = (blockIdx.x / nseg) % OH, img = blockIdx.x / (nseg * OH);
    const int b = img % B;
    if (origins) {
        // device-side metadata, clamped so that nothing below can overflow: an origin outside the frame shows zeros, as one inside shows the frame
        int oy = origins[2 * (img / B)], ox = origins[2 * (img / B) + 1];
        oy = oy < -OH ? -OH : (oy > h ? h : oy);
        ox = ox < -OW ? -OW : (ox > w ? w : ox);
        y0 = -oy; x0 = -ox;
    }
    const int c0 = seg * SEG, c1 = c0 + SEG < OW ? c0 + SEG : OW;
    const int sy = row - y0;
    const int px_lo = c0 - x0 > 0 ? c0 - x0 : 0, px_hi = c1 - x0 < w ? c1 - x0 : w;
    const int n = px_hi - px_lo;
    const bool live = sy >= 0 && sy < h && n > 0;                    // workgroup-uniform
    const unsigned char* g0 = reinterpret_cast<const unsigned char*>(src);
    if (live) {
        if (hwc) {
            run_to_lds(g0 + (((size_t)b * h + sy) * w + px_lo) * C * sizeof(S), lds, n * C * (int)sizeof(S));
        } else {
            for (int c = 0; c < C; ++c) run_to_lds(g0 + ((((size_t)b * C + c) * h + sy) * w + px_lo) * sizeof(S), lds + c * REG, n * (int)sizeof(S));
        }
        __syncthreads();
    }
    const int col = c0 + 4 * (int)threadIdx.x;
    if (col >= c1) return;
    float in4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) in4[j] = (live && col + j - x0 >= px_lo && col + j - x0 < px_hi) ? 1.0f : 0.0f;
    const int sh_hwc = (int)((uintptr_t)(g0 + (((size_t)b * h + (live ? sy : 0)) * w + px_lo) * C * sizeof(S)) & 15);
    for (int c = 0; c < C; ++c) {
        const int cs = swapped(c, swap_rb);
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (live) {
            const int sh_chw = (int)((uintptr_t)(g0 + ((((size_t)b * C + cs) * h + sy) * w + px_lo) * sizeof(S)) & 15);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (in4[j] != 0.0f) {
                    const int px = col + j - x0 - px_lo;
                    const unsigned char* p = hwc ? lds + sh_hwc + ((size_t)px * C + cs) * sizeof(S) : lds + cs * REG + sh_chw + (size_t)px * sizeof(S);
                    v[j] = to_unit(*reinterpret_cast<const S*>(p));
                }
            }
        }
        float* o = out + (((size_t)img * C + c) * OH + row) * OW + col;
        if constexpr (VEC) {
            *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) if (col + j < c1) o[j] = v[j];
        }
    }
    if (mask) {
        float* o = mask + ((size_t)img * OH + row) * OW + col;
        if constexpr (VEC) {
            *reinterpret_cast<f32x4*>(o) = f32x4{in4[0], in4[1], in4[2], in4[3]};
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) if (col + j < c1) o[j] = in4[j];
        }
    }
}

// ---- canvas -> frames ------------------------------------------------------------------------------------------------------------------
// frames (B,h,w,C) or (B,C,h,w) u8 = quantise(canvas[:, :, y0:y0+h, x0:x0+w]); a segment is SEG canvas columns from a0 = x0 rounded down to
// a multiple of 4 (VEC) or x0, so that a lane's four columns are one aligned 16-byte load
template <bool VEC>
__global__ __launch_bounds__(256) void quantise_rows_kernel(const float* __restrict__ canvas, unsigned char* __restrict__ frames, int hwc, int swap_rb, int B, int C,
                                                            int h, int w, int Xh, int Xw, int y0, int x0, int nseg) {
    constexpr int REG = SEG + 16;
    __shared__ __attribute__((aligned(16))) unsigned char lds[MAX_C_U8 * REG];
    const int seg = blockIdx.x % nseg, y = (blockIdx.x / nseg) % h, b = blockIdx.x / (nseg * h);
    const int a0 = VEC ? (x0 & ~3) : x0;
    const int c0 = a0 + seg * SEG;
    const int lo = c0 > x0 ? c0 : x0, hi = c0 + SEG < x0 + w ? c0 + SEG : x0 + w;
    const int px_lo = lo - x0, n = hi - lo;                           // n > 0 by the choice of nseg
    unsigned char* g_hwc = frames + (((size_t)b * h + y) * w + px_lo) * C;
    const int sh_hwc = (int)((uintptr_t)g_hwc & 15);
    const int col = c0 + 4 * (int)threadIdx.x;
    if (col < hi) {
        for (int c = 0; c < C; ++c) {
            const int cs = swapped(c, swap_rb);
            const float* p = canvas + (((size_t)b * C + cs) * Xh + y0 + y) * Xw + col;
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if constexpr (VEC) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(p);  // col % 4 == 0 and Xw % 4 == 0: the four columns are in the row
                v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) if (col + j < hi) v[j] = p[j];
            }
            unsigned char* g_chw = frames + (((size_t)b * C + c) * h + y) * w + px_lo;
            const int sh_chw = (int)((uintptr_t)g_chw & 15);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (col + j >= lo && col + j < hi) {
                    const int px = col + j - lo;
                    if (hwc) lds[sh_hwc + px * C + c] = quantise(v[j]); else lds[c * REG + sh_chw + px] = quantise(v[j]);
                }
            }
        }
    }
    __syncthreads();
    if (hwc) {
        lds_to_run(lds, g_hwc, n * C);
    } else {
        for (int c = 0; c < C; ++c) lds_to_run(lds + c * REG, frames + (((size_t)b * C + c) * h + y) * w + px_lo, n);
    }
}

// ---- tiles -> frame --------------------------------------------------------------------------------------------------------------------
struct Starts { int ys[MAX_STARTS]; int xs[MAX_STARTS]; int ny, nx; };

// infer.restore_tiled's ramp() in closed form: the weight of tile i of `s` at coordinate p of an axis of length len
__device__ __forceinline__ float axis_weight(const int* s, int n, int i, int p, int len, int tile) {
    const int start = s[i];
    const int size = tile < len - start ? tile : len - start;
    const int r = p - start;
    float wgt = 1.0f;
    if (i > 0) {
        const int ov = s[i - 1] + tile - start;
        if (ov > 0 && r < ov) wgt = ((float)r + 0.5f) / (float)ov;
    }
    if (i + 1 < n) {
        const int ov = start + tile - s[i + 1];
        if (ov > 0 && r >= size - ov) wgt = wgt * (1.0f - ((float)(r - (size - ov)) + 0.5f) / (float)ov);
    }
    return wgt;
}

// out(b,c,y,x) = sum_t w_t o_t / sum_t w_t over every tile t = (ty,tx) that holds (y,x), ascending t = ty * nx + tx, f32; tile t of frame b is
// image t * B + b of tiles.  U8: frames (B,h,w,C) / (B,C,h,w) through quantise(); else f32 planes (B,C,h,w), clamped to [0,1] on request
template <bool U8>
__global__ __launch_bounds__(256) void blend_rows_kernel(const float* __restrict__ tiles, const Starts st, void* __restrict__ outp, int hwc, int swap_rb, int clamp01,
                                                         int B, int C, int h, int w, int tile, int nseg) {
#pragma clang fp contract(off)
    constexpr int REG = SEG + 16;
    __shared__ __attribute__((aligned(16))) unsigned char lds[U8 ? MAX_C_U8 * REG : 16];
    const int seg = blockIdx.x % nseg, y = (blockIdx.x / nseg) % h, b = blockIdx.x / (nseg * h);
    const int px_lo = seg * SEG, n = px_lo + SEG < w ? SEG : w - px_lo;
    unsigned char* frames = reinterpret_cast<unsigned char*>(outp);
    float* planes = reinterpret_cast<float*>(outp);
    unsigned char* g_hwc = frames + (((size_t)b * h + y) * w + px_lo) * C;
    const int sh_hwc = (int)((uintptr_t)g_hwc & 15);
    const size_t plane = (size_t)tile * tile;
    for (int px = threadIdx.x; px < n; px += 256) {
        const int x = px_lo + px;
        float num[MAX_C], den = 0.0f;
#pragma unroll
        for (int c = 0; c < MAX_C; ++c) num[c] = 0.0f;
        for (int ty = 0; ty < st.ny; ++ty) {
            if (y < st.ys[ty] || y >= st.ys[ty] + tile) continue;    // workgroup-uniform
            const float wy = axis_weight(st.ys, st.ny, ty, y, h, tile);
            for (int tx = 0; tx < st.nx; ++tx) {
                if (x < st.xs[tx] || x >= st.xs[tx] + tile) continue;
                const float wgt = wy * axis_weight(st.xs, st.nx, tx, x, w, tile);
                const float* o = tiles + ((size_t)(ty * st.nx + tx) * B + b) * C * plane + (size_t)(y - st.ys[ty]) * tile + (x - st.xs[tx]);
                den += wgt;
#pragma unroll
                for (int c = 0; c < MAX_C; ++c) if (c < C) num[c] += o[c * plane] * wgt;
            }
        }
#pragma unroll
        for (int c = 0; c < MAX_C; ++c) {
            if (c >= C) continue;
            const int cs = swapped(c, swap_rb);
            float v = 0.0f;
#pragma unroll
            for (int k = 0; k < MAX_C; ++k) if (k == cs) v = num[k];
            v = v / den;
            if constexpr (U8) {
                if (hwc) {
                    lds[sh_hwc + px * C + c] = quantise(v);
                } else {
                    const int sh_chw = (int)((uintptr_t)(frames + (((size_t)b * C + c) * h + y) * w + px_lo) & 15);
                    lds[c * REG + sh_chw + px] = quantise(v);
                }
            } else {
                if (clamp01) v = v != v ? v : fminf(fmaxf(v, 0.0f), 1.0f);   // torch.clamp: NaN stays NaN
                planes[(((size_t)b * C + c) * h + y) * w + x] = v;
            }
        }
    }
    if constexpr (U8) {
        __syncthreads();
        if (hwc) {
            lds_to_run(lds, g_hwc, n * C);
        } else {
            for (int c = 0; c < C; ++c) lds_to_run(lds + c * REG, frames + (((size_t)b * C + c) * h + y) * w + px_lo, n);
        }
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <typename S>
void launch_paste(const void* src, int hwc, int swap_rb, float* out, float* mask, const int* origins, int B, int C, int h, int w, int NI, int OH, int OW, int y0, int x0,
                  hipStream_t st) {
    const int nseg = (OW + SEG - 1) / SEG;
    const dim3 grid((unsigned)((long long)NI * OH * nseg));
    if (OW % 4 == 0 && aligned16(out) && aligned16(mask))
        hipLaunchKernelGGL((paste_rows_kernel<S, true>), grid, dim3(256), 0, st, (const S*)src, hwc, swap_rb, out, mask, origins, B, C, h, w, OH, OW, y0, x0, nseg);
    else
        hipLaunchKernelGGL((paste_rows_kernel<S, false>), grid, dim3(256), 0, st, (const S*)src, hwc, swap_rb, out, mask, origins, B, C, h, w, OH, OW, y0, x0, nseg);
}

}  // namespace
}  // namespace uf

using namespace uf;

extern "C" int uf_frames_to_canvas(const uint8_t* frames, int hwc, int swap_rb, float* canvas, float* mask, int B, int C, int h, int w, int Xh, int Xw, void* stream) {
    UF_REQUIRE(frames && canvas, UF_ERR_NULL, "uf_frames_to_canvas: null pointer");
    UF_REQUIRE(C >= 1 && C <= MAX_C, UF_ERR_UNSUPPORTED, "uf_frames_to_canvas: C=%d (1 ... %d channels)", C, MAX_C);
    UF_REQUIRE(!swap_rb || C >= 3, UF_ERR_UNSUPPORTED, "uf_frames_to_canvas: swap_rb needs C >= 3, got C=%d", C);
    UF_REQUIRE(B > 0 && h > 0 && w > 0, UF_ERR_SHAPE, "uf_frames_to_canvas: B=%d h=%d w=%d", B, h, w);
    UF_REQUIRE(Xh >= h && Xw >= w, UF_ERR_SHAPE, "uf_frames_to_canvas: canvas Xh=%d Xw=%d smaller than the image h=%d w=%d", Xh, Xw, h, w);
    const long long nseg = (Xw + SEG - 1) / SEG;
    UF_REQUIRE((long long)B * C * Xh * Xw < LIMIT31 && (long long)B * Xh * nseg < LIMIT31, UF_ERR_SHAPE,
               "uf_frames_to_canvas: B*C*Xh*Xw = %lld canvas elements, the limit is 2^31", (long long)B * C * Xh * Xw);
    hipStream_t st = (hipStream_t)stream;
    {
        ScopedTimer tm("frames_to_canvas", 0.0, 4.0 * B * (C + (mask ? 1 : 0)) * Xh * Xw + 1.0 * B * C * h * w, st);
        launch_paste<unsigned char>(frames, hwc, swap_rb, canvas, mask, nullptr, B, C, h, w, B, Xh, Xw, (Xh - h) / 2, (Xw - w) / 2, st);
    }
    return check_launch("frames_to_canvas");
}

extern "C" int uf_canvas_to_frames(const float* canvas, uint8_t* frames, int hwc, int swap_rb, int B, int C, int h, int w, int Xh, int Xw, void* stream) {
    UF_REQUIRE(canvas && frames, UF_ERR_NULL, "uf_canvas_to_frames: null pointer");
    UF_REQUIRE(C >= 1 && C <= MAX_C_U8, UF_ERR_UNSUPPORTED, "uf_canvas_to_frames: C=%d (1 ... %d channels)", C, MAX_C_U8);
    UF_REQUIRE(!swap_rb || C >= 3, UF_ERR_UNSUPPORTED, "uf_canvas_to_frames: swap_rb needs C >= 3, got C=%d", C);
    UF_REQUIRE(B > 0 && h > 0 && w > 0, UF_ERR_SHAPE, "uf_canvas_to_frames: B=%d h=%d w=%d", B, h, w);
    UF_REQUIRE(Xh >= h && Xw >= w, UF_ERR_SHAPE, "uf_canvas_to_frames: canvas Xh=%d Xw=%d smaller than the image h=%d w=%d", Xh, Xw, h, w);
    UF_REQUIRE((long long)B * C * Xh * Xw < LIMIT31, UF_ERR_SHAPE, "uf_canvas_to_frames: B*C*Xh*Xw = %lld canvas elements, the limit is 2^31",
               (long long)B * C * Xh * Xw);
    const int y0 = (Xh - h) / 2, x0 = (Xw - w) / 2;
    const bool vec = Xw % 4 == 0 && aligned16(canvas);
    const int a0 = vec ? (x0 & ~3) : x0;
    const int nseg = (x0 + w - a0 + SEG - 1) / SEG;
    const dim3 grid((unsigned)((long long)B * h * nseg));
    hipStream_t st = (hipStream_t)stream;
    {
        ScopedTimer tm("canvas_to_frames", 0.0, 5.0 * B * C * h * w, st);
        if (vec) hipLaunchKernelGGL(quantise_rows_kernel<true>, grid, dim3(256), 0, st, canvas, frames, hwc, swap_rb, B, C, h, w, Xh, Xw, y0, x0, nseg);
        else hipLaunchKernelGGL(quantise_rows_kernel<false>, grid, dim3(256), 0, st, canvas, frames, hwc, swap_rb, B, C, h, w, Xh, Xw, y0, x0, nseg);
    }
    return check_launch("canvas_to_frames");
}

extern "C" int uf_tiles_gather(const void* src, int src_is_u8, int src_hwc, int swap_rb, float* tiles, const int* origins, int T, int B, int C, int h, int w, int tile,
                               void* stream) {
    UF_REQUIRE(src && tiles && origins, UF_ERR_NULL, "uf_tiles_gather: null pointer");
    UF_REQUIRE(C >= 1 && C <= MAX_C, UF_ERR_UNSUPPORTED, "uf_tiles_gather: C=%d (1 ... %d channels)", C, MAX_C);
    UF_REQUIRE(!swap_rb || C >= 3, UF_ERR_UNSUPPORTED, "uf_tiles_gather: swap_rb needs C >= 3, got C=%d", C);
    UF_REQUIRE(tile > 0 && tile % 128 == 0, UF_ERR_SHAPE, "uf_tiles_gather: tile=%d must be a multiple of 128", tile);
    UF_REQUIRE(T > 0 && B > 0 && h > 0 && w > 0, UF_ERR_SHAPE, "uf_tiles_gather: T=%d B=%d h=%d w=%d", T, B, h, w);
    const long long n = (long long)T * B * C * tile * tile;
    UF_REQUIRE(n < LIMIT31 && (long long)B * C * h * w * (src_is_u8 ? 1 : 4) < LIMIT31, UF_ERR_SHAPE,
               "uf_tiles_gather: T*B*C*tile*tile = %lld tile elements, B*C*h*w = %lld frame elements, the limit is 2^31 elements / bytes", n, (long long)B * C * h * w);
    hipStream_t st = (hipStream_t)stream;
    {
        ScopedTimer tm("tiles_gather", 0.0, 4.0 * n + (src_is_u8 ? 1.0 : 4.0) * B * C * h * w, st);
        if (src_is_u8) launch_paste<unsigned char>(src, src_hwc, swap_rb, tiles, nullptr, origins, B, C, h, w, T * B, tile, tile, 0, 0, st);
        else launch_paste<float>(src, src_hwc, swap_rb, tiles, nullptr, origins, B, C, h, w, T * B, tile, tile, 0, 0, st);
    }
    return check_launch("tiles_gather");
}

extern "C" int uf_tiles_blend(const float* tiles_out, const int* ys, int ny, const int* xs, int nx, void* out, int out_is_u8, int out_hwc, int swap_rb, int clamp01,
                              int B, int C, int h, int w, int tile, void* stream) {
    UF_REQUIRE(tiles_out && ys && xs && out, UF_ERR_NULL, "uf_tiles_blend: null pointer");
    const int max_c = out_is_u8 ? MAX_C_U8 : MAX_C;
    UF_REQUIRE(C >= 1 && C <= max_c, UF_ERR_UNSUPPORTED, "uf_tiles_blend: C=%d (1 ... %d channels for %s output)", C, max_c, out_is_u8 ? "u8" : "f32");
    UF_REQUIRE(!swap_rb || C >= 3, UF_ERR_UNSUPPORTED, "uf_tiles_blend: swap_rb needs C >= 3, got C=%d", C);
    UF_REQUIRE(tile > 0 && tile % 128 == 0, UF_ERR_SHAPE, "uf_tiles_blend: tile=%d must be a multiple of 128", tile);
    UF_REQUIRE(B > 0 && h > 0 && w > 0, UF_ERR_SHAPE, "uf_tiles_blend: B=%d h=%d w=%d", B, h, w);
    UF_REQUIRE(ny >= 1 && ny <= MAX_STARTS && nx >= 1 && nx <= MAX_STARTS, UF_ERR_SHAPE, "uf_tiles_blend: ny=%d nx=%d (1 ... %d starts per axis)", ny, nx, MAX_STARTS);
    Starts s{};
    s.ny = ny; s.nx = nx;
    for (int a = 0; a < 2; ++a) {
        const int* v = a ? xs : ys;
        const int n = a ? nx : ny, len = a ? w : h;
        // every pixel lies in a tile: the starts begin at 0, ascend by at most a tile and reach the far side
        bool ok = v[0] == 0 && v[n - 1] < len && v[n - 1] + tile >= len;
        for (int i = 0; ok && i + 1 < n; ++i) ok = v[i + 1] > v[i] && v[i + 1] - v[i] <= tile;
        UF_REQUIRE(ok, UF_ERR_SHAPE, "uf_tiles_blend: the %s starts do not cover 0 ... %d in ascending tiles of %d", a ? "x" : "y", len, tile);
        for (int i = 0; i < n; ++i) (a ? s.xs : s.ys)[i] = v[i];
    }
    const long long n = (long long)ny * nx * B * C * tile * tile;
    const int nseg = (w + SEG - 1) / SEG;
    UF_REQUIRE(n < LIMIT31 && (long long)B * C * h * w < LIMIT31 && (long long)B * h * nseg < LIMIT31, UF_ERR_SHAPE,
               "uf_tiles_blend: ny*nx*B*C*tile*tile = %lld tile elements, B*C*h*w = %lld frame elements, the limit is 2^31", n, (long long)B * C * h * w);
    const dim3 grid((unsigned)((long long)B * h * nseg));
    hipStream_t st = (hipStream_t)stream;
    {
        ScopedTimer tm("tiles_blend", 0.0, 4.0 * n + (out_is_u8 ? 1.0 : 4.0) * B * C * h * w, st);
        if (out_is_u8) hipLaunchKernelGGL(blend_rows_kernel<true>, grid, dim3(256), 0, st, tiles_out, s, out, out_hwc, swap_rb, clamp01, B, C, h, w, tile, nseg);
        else hipLaunchKernelGGL(blend_rows_kernel<false>, grid, dim3(256), 0, st, tiles_out, s, out, out_hwc, swap_rb, clamp01, B, C, h, w, tile, nseg);
    }
    return check_launch("tiles_blend");
}
