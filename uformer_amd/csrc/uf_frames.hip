// uint8 frames in and out of the model on the device: the conversions either side of infer.restore / infer.restore_tiled as
// byte-moving kernels, none with matrix work; and the member batch and the mean of the geometric self-ensemble.
//   uf_frames_to_canvas   u8 frames (interleaved or planar) -> zero-padded f32 canvas (+ mask), u / 255 like load_img (utils/image_utils.py:31-35)
//   uf_canvas_to_frames   crop + clamp + quantise: img_as_ubyte(clamp(x, 0, 1)) of test/test_gopro_hide.py:103-110 for float32 input
//   uf_tiles_gather       the tile batch of infer.restore_tiled (torch.cat(tiles, 0)) from u8 or f32 frames
//   uf_tiles_blend        the ramp-weighted sum of the restored tiles over the sum of the weights, as f32 planes or u8 frames
//   uf_tta_gather         the padded members T_k(frame) of infer.restore_ensemble as one batch, from u8 or f32 frames
//   uf_tta_merge          the balanced pairwise mean of the restored members turned back, as f32 planes or u8 frames
// One workgroup owns one output row segment of SEG columns.  The frame side of a segment is one run of bytes (interleaved) or one run per channel
// (planar): it moves between global memory and LDS as 16-byte accesses over the aligned body of the run and single bytes over the < 16 at each end,
// at the LDS offset that has the global address's low four bits, so that both sides of every 16-byte copy are aligned for any row length and any
// channel count.  The f32 side is read and written four columns per lane (one 16-byte access) when the row pitch and the base pointer allow it.
// The transposition between the two layouts is the LDS access pattern.  The u8 results reach memory as the dwords assembled in LDS.
#include <initializer_list>

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
// one output row segment: seg, row, img say which; (fy, fx) show the frame flipped along y / x (0, 0: as it is)
template <typename S, bool VEC>
__device__ __forceinline__ void paste_row(const S* __restrict__ src, int hwc, int swap_rb, float* __restrict__ out, float* __restrict__ mask, unsigned char* lds, int b, int img,
                                          int seg, int row, int C, int h, int w, int OH, int OW, int y0, int x0, int fy, int fx) {
    constexpr int REG = SEG * (int)sizeof(S) + 16;                   // bytes of LDS per planar channel run
    const int c0 = seg * SEG, c1 = c0 + SEG < OW ? c0 + SEG : OW;
    const int iy = row - y0;
    const int sy = fy ? h - 1 - iy : iy;
    const int px_lo = c0 - x0 > 0 ? c0 - x0 : 0, px_hi = c1 - x0 < w ? c1 - x0 : w;
    const int n = px_hi - px_lo;
    const int s_lo = fx ? w - px_hi : px_lo;                         // the run's first source column
    const bool live = iy >= 0 && iy < h && n > 0;                    // workgroup-uniform
    const unsigned char* g0 = reinterpret_cast<const unsigned char*>(src);
    if (live) {
        if (hwc) {
            run_to_lds(g0 + (((size_t)b * h + sy) * w + s_lo) * C * sizeof(S), lds, n * C * (int)sizeof(S));
        } else {
            for (int c = 0; c < C; ++c) run_to_lds(g0 + ((((size_t)b * C + c) * h + sy) * w + s_lo) * sizeof(S), lds + c * REG, n * (int)sizeof(S));
        }
        __syncthreads();
    }
    const int col = c0 + 4 * (int)threadIdx.x;
    if (col >= c1) return;
    float in4[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) in4[j] = (live && col + j - x0 >= px_lo && col + j - x0 < px_hi) ? 1.0f : 0.0f;
    const int sh_hwc = (int)((uintptr_t)(g0 + (((size_t)b * h + (live ? sy : 0)) * w + s_lo) * C * sizeof(S)) & 15);
    for (int c = 0; c < C; ++c) {
        const int cs = swapped(c, swap_rb);
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (live) {
            const int sh_chw = (int)((uintptr_t)(g0 + ((((size_t)b * C + cs) * h + sy) * w + s_lo) * sizeof(S)) & 15);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (in4[j] != 0.0f) {
                    const int pi = col + j - x0 - px_lo;
                    const int px = fx ? n - 1 - pi : pi;
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

template <typename S, bool VEC>
__global__ __launch_bounds__(256) void paste_rows_kernel(const S* __restrict__ src, int hwc, int swap_rb, float* __restrict__ out, float* __restrict__ mask,
                                                         const int* __restrict__ origins, int B, int C, int h, int w, int OH, int OW, int y0, int x0, int nseg) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[MAX_C * (SEG * (int)sizeof(S) + 16)];
    const int seg = blockIdx.x % nseg, row = (blockIdx.x / nseg) % OH, img = blockIdx.x / (nseg * OH);
    if (origins) {
        // device-side metadata, clamped so that nothing below can overflow: an origin outside the frame shows zeros, as one inside shows the frame
        int oy = origins[2 * (img / B)], ox = origins[2 * (img / B) + 1];
        oy = oy < -OH ? -OH : (oy > h ? h : oy);
        ox = ox < -OW ? -OW : (ox > w ? w : ox);
        y0 = -oy; x0 = -ox;
    }
    paste_row<S, VEC>(src, hwc, swap_rb, out, mask, lds, img % B, img, seg, row, C, h, w, OH, OW, y0, x0, 0, 0);
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

// ---- self-ensemble: the eight flips and rotations as one batch ------------------------------------------------------
// T_k = Augment_RGB_torch.transform<k> of an (h, w) image, member(my, mx) = img(sy, sx):
//   even k: (h, w) member,  sy = fy ? h-1-my : my,  sx = fx ? w-1-mx : mx
//   odd k:  (w, h) member,  sy = fy ? h-1-mx : mx,  sx = fx ? w-1-my : my
// with fy set for k = 1, 2, 4, 5 and fx for k = 2, 3, 5, 6 (crop_aug_kernel's table in this form).  A list of members travels as one kernel
// argument, four bits each.
constexpr int TG = 64;                  // tile side of the transposing gather
constexpr int TM = 32;                  // tile side of the merge
__device__ __forceinline__ int flips_y(int k) { return (0x36 >> k) & 1; }
__device__ __forceinline__ int flips_x(int k) { return (0x6C >> k) & 1; }

// even members: out (n*B, C, Xh, Xw), image m * B + b = frame b under T_ks[m], centred; paste_row with the row and the columns mirrored
template <typename S, bool VEC>
__global__ __launch_bounds__(256) void tta_rows_kernel(const S* __restrict__ src, int hwc, int swap_rb, float* __restrict__ out, unsigned ks, int B, int C, int h, int w,
                                                       int Xh, int Xw, int nseg) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[MAX_C * (SEG * (int)sizeof(S) + 16)];
    const int seg = blockIdx.x % nseg, row = (blockIdx.x / nseg) % Xh, img = blockIdx.x / (nseg * Xh);
    const int k = (ks >> (4 * (img / B))) & 7;
    paste_row<S, VEC>(src, hwc, swap_rb, out, nullptr, lds, img % B, img, seg, row, C, h, w, Xh, Xw, (Xh - h) / 2, (Xw - w) / 2, flips_y(k), flips_x(k));
}

// odd members: one workgroup per TG x TG tile of a canvas plane.  The source rectangle of the tile is read along the source rows (lane = source
// column) into an LDS tile of pitch TG + 1 and leaves along the canvas rows (lane = canvas column = source row): both global sides are coalesced,
// both LDS sides conflict-free.  Canvas elements outside the member are written as zeros by the same stores.
template <typename S>
__global__ __launch_bounds__(256) void tta_transpose_kernel(const S* __restrict__ src, int hwc, int swap_rb, float* __restrict__ out, unsigned ks, int B, int C, int h, int w,
                                                            int Xh, int Xw, int ntx, int nty) {
    __shared__ float tile[TG][TG + 1];
    const int tx0 = (blockIdx.x % ntx) * TG, ty0 = ((blockIdx.x / ntx) % nty) * TG, img = blockIdx.x / (ntx * nty);
    const int b = img % B, k = (ks >> (4 * (img / B))) & 7;
    const int fy = flips_y(k), fx = flips_x(k);
    const int y0 = (Xh - w) / 2, x0 = (Xw - h) / 2;                   // the member is (w, h)
    const int my_lo = ty0 - y0 > 0 ? ty0 - y0 : 0, my_hi = ty0 + TG - y0 < w ? ty0 + TG - y0 : w;
    const int mx_lo = tx0 - x0 > 0 ? tx0 - x0 : 0, mx_hi = tx0 + TG - x0 < h ? tx0 + TG - x0 : h;
    const int ny = my_hi - my_lo, nx = mx_hi - mx_lo;                 // source columns, source rows of this tile
    const bool live = ny > 0 && nx > 0;                               // workgroup-uniform
    const int sy_lo = fy ? h - mx_hi : mx_lo, sx_lo = fx ? w - my_hi : my_lo;
    const int i = threadIdx.x % TG, r = threadIdx.x / TG;
    for (int c = 0; c < C; ++c) {
        const int cs = swapped(c, swap_rb);
        if (live) {
            if (i < ny) {
                for (int rr = r; rr < nx; rr += 256 / TG) {
                    const size_t at = hwc ? (((size_t)b * h + sy_lo + rr) * w + sx_lo + i) * C + cs : (((size_t)b * C + cs) * h + sy_lo + rr) * w + sx_lo + i;
                    tile[rr][i] = to_unit(src[at]);
                }
            }
            __syncthreads();
        }
        const int ox = tx0 + i, mx = ox - x0;
        if (ox < Xw) {
            for (int rr = r; rr < TG && ty0 + rr < Xh; rr += 256 / TG) {
                const int my = ty0 + rr - y0;
                float v = 0.0f;
                if (live && my >= my_lo && my < my_hi && mx >= mx_lo && mx < mx_hi) v = tile[(fy ? h - 1 - mx : mx) - sy_lo][(fx ? w - 1 - my : my) - sx_lo];
                out[(((size_t)img * C + c) * Xh + ty0 + rr) * Xw + ox] = v;
            }
        }
        if (live) __syncthreads();
    }
}

// the members of a merge in ascending k, decoded on the host: nothing about a member is worked out per pixel
struct MergePlan {
    long long base[8];                  // even: offset of the element that output pixel (0,0) of frame 0, channel 0 reads; odd: of the member's region
    int dy[8], dx[8];                   // even: element steps per output row and column (+-Xw, +-1); odd: fy, fx of the member
    int slot[8];                        // odd: its LDS tile; -1 for an even member
    int staged;                         // any odd member
};
constexpr int MERGE_UNROLL = 1;         // pixels a lane has in flight: 1 and 2 measure the same, 4 (all of a channel's) is 1.6 x slower

// out = clamp01(tree_sum_k T_k^-1(crop_k(y_k)) / n): one workgroup per TM x TM tile of the output, all channels.  An even member is read in place
// (along canvas rows, mirrored or not); an odd member's rectangle goes through an LDS tile as in tta_transpose_kernel.  The balanced pairwise sum
// ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) is held in registers.  U8: frames through quantise(), assembled in LDS and stored as runs of bytes.
template <bool U8, int N>
__global__ __launch_bounds__(256) void tta_merge_kernel(const float* __restrict__ even, int Xh, int Xw, const float* __restrict__ odd, int Xoh, int Xow,
                                                        const MergePlan p, float scale, void* __restrict__ outp, int hwc, int swap_rb, int clamp01,
                                                        int B, int C, int h, int w, int ntx, int nty) {
    __shared__ float tile[4][TM][TM + 1];
    __shared__ unsigned char q[U8 ? MAX_C_U8 * TM * TM : 16];
    const int x0t = (blockIdx.x % ntx) * TM, y0t = ((blockIdx.x / ntx) % nty) * TM, b = blockIdx.x / (ntx * nty);
    const int tw = x0t + TM < w ? TM : w - x0t, th = y0t + TM < h ? TM : h - y0t;
    const int i = threadIdx.x % TM, r = threadIdx.x / TM;
    const size_t plane_e = (size_t)Xh * Xw, plane_o = (size_t)Xoh * Xow;
    for (int c = 0; c < C; ++c) {
        const int cs = swapped(c, swap_rb);
        if (p.staged) {
#pragma unroll
            for (int j = 0; j < N; ++j) {
                if (p.slot[j] < 0) continue;
                // rows my = fx ? w-1-x : x over the tile's columns, columns mx = fy ? h-1-y : y over its rows
                const int my_lo = p.dx[j] ? w - (x0t + tw) : x0t, mx_lo = p.dy[j] ? h - (y0t + th) : y0t;
                const float* src = odd + p.base[j] + ((size_t)b * C + cs) * plane_o + (size_t)my_lo * Xow + mx_lo;
                if (i < th) for (int rr = r; rr < tw; rr += 256 / TM) tile[p.slot[j]][rr][i] = src[(size_t)rr * Xow + i];
            }
            __syncthreads();
        }
        const float* ev = even + ((size_t)b * C + cs) * plane_e;
#pragma unroll(MERGE_UNROLL)
        for (int jj = 0; jj < TM * TM / 256; ++jj) {
            const int yl = r + (256 / TM) * jj;
            if (yl >= th || i >= tw) continue;
            const int y = y0t + yl, x = x0t + i;
            float v[N];
#pragma unroll
            for (int j = 0; j < N; ++j) {
                if (p.slot[j] >= 0) v[j] = tile[p.slot[j]][p.dx[j] ? tw - 1 - i : i][p.dy[j] ? th - 1 - yl : yl];
                else v[j] = ev[p.base[j] + (long long)y * p.dy[j] + x * p.dx[j]];
            }
#pragma unroll
            for (int s = N; s > 1; s >>= 1) {
#pragma unroll
                for (int j = 0; j < s / 2; ++j) v[j] = v[2 * j] + v[2 * j + 1];
            }
            const float res = v[0] * scale;
            if constexpr (U8) {
                q[hwc ? (yl * TM + i) * C + c : (c * TM + yl) * TM + i] = quantise(res);
            } else {
                reinterpret_cast<float*>(outp)[(((size_t)b * C + c) * h + y) * w + x] = clamp01 ? (res < 0.f ? 0.f : (res > 1.f ? 1.f : res)) : res;   // NaN stays NaN
            }
        }
        if (p.staged) __syncthreads();
    }
    if constexpr (U8) {
        unsigned char* frames = reinterpret_cast<unsigned char*>(outp);
        __syncthreads();
        if (hwc) {
            const int run = tw * C;
            for (int e = threadIdx.x; e < th * run; e += 256) {
                const int yl = e / run, j = e % run;
                frames[(((size_t)b * h + y0t + yl) * w + x0t) * C + j] = q[yl * TM * C + j];
            }
        } else {
            for (int e = threadIdx.x; e < C * th * tw; e += 256) {
                const int cc = e / (th * tw), yl = (e / tw) % th, j = e % tw;
                frames[(((size_t)b * C + cc) * h + y0t + yl) * w + x0t + j] = q[(cc * TM + yl) * TM + j];
            }
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

namespace {
// a member list as the kernels take it: distinct k in 0 ... 7, ascending, of one parity.  0 when it is one, else the status and the message
// the product of positive ints, or 2^31 as soon as it reaches that: no factor list can overflow it
long long capped_product(std::initializer_list<int> f) {
    long long v = 1;
    for (const int x : f) {
        v *= x;
        if (v >= LIMIT31) return LIMIT31;
    }
    return v;
}
int check_members(const char* who, const char* what, const int* ks, int n, int parity /* -1: either */) {
    for (int i = 0; i < n; ++i) {
        UF_REQUIRE(ks[i] >= 0 && ks[i] <= 7, UF_ERR_UNSUPPORTED, "%s: %s[%d]=%d (a transform is 0 ... 7)", who, what, i, ks[i]);
        UF_REQUIRE(i == 0 || ks[i] > ks[i - 1], UF_ERR_UNSUPPORTED, "%s: %s must be distinct and ascending, got %d after %d", who, what, ks[i], ks[i - 1]);
        UF_REQUIRE((ks[i] & 1) == (parity < 0 ? (ks[0] & 1) : parity), UF_ERR_UNSUPPORTED, "%s: %s mixes parities (%d beside %d): one canvas shape per list", who, what, ks[i],
                   parity < 0 ? ks[0] : parity);
    }
    return UF_OK;
}
}  // namespace

extern "C" int uf_tta_gather(const void* src, int src_is_u8, int src_hwc, int swap_rb, float* out, const int* ks, int n, int B, int C, int h, int w, int Xh, int Xw,
                             void* stream) {
    UF_REQUIRE(src && out && ks, UF_ERR_NULL, "uf_tta_gather: null pointer");
    UF_REQUIRE(C >= 1 && C <= MAX_C, UF_ERR_UNSUPPORTED, "uf_tta_gather: C=%d (1 ... %d channels)", C, MAX_C);
    UF_REQUIRE(!swap_rb || C >= 3, UF_ERR_UNSUPPORTED, "uf_tta_gather: swap_rb needs C >= 3, got C=%d", C);
    UF_REQUIRE(n == 1 || n == 2 || n == 4 || n == 8, UF_ERR_UNSUPPORTED, "uf_tta_gather: n=%d members (1, 2, 4 or 8)", n);
    if (const int rc = check_members("uf_tta_gather", "ks", ks, n, -1)) return rc;
    UF_REQUIRE(B > 0 && h > 0 && w > 0, UF_ERR_SHAPE, "uf_tta_gather: B=%d h=%d w=%d", B, h, w);
    const bool odd = ks[0] & 1;
    const int hk = odd ? w : h, wk = odd ? h : w;
    UF_REQUIRE(Xh >= hk && Xw >= wk, UF_ERR_SHAPE, "uf_tta_gather: canvas Xh=%d Xw=%d smaller than the member h=%d w=%d", Xh, Xw, hk, wk);
    const long long total = capped_product({n, B, C, Xh, Xw}), frame = capped_product({B, C, h, w, src_is_u8 ? 1 : 4});
    const long long blocks = odd ? capped_product({n, B, (Xh - 1) / TG + 1, (Xw - 1) / TG + 1}) : capped_product({n, B, Xh, (Xw - 1) / SEG + 1});
    UF_REQUIRE(total < LIMIT31 && blocks < LIMIT31 && frame < LIMIT31, UF_ERR_SHAPE,
               "uf_tta_gather: n*B*C*Xh*Xw = %lld canvas elements, B*C*h*w = %lld frame bytes (2^31 stands for more), the limit is 2^31 elements / bytes", total, frame);
    unsigned packed = 0;
    for (int i = 0; i < n; ++i) packed |= (unsigned)ks[i] << (4 * i);
    hipStream_t st = (hipStream_t)stream;
    {
        ScopedTimer tm("tta_gather", 0.0, 4.0 * total + (src_is_u8 ? 1.0 : 4.0) * n * B * C * h * w, st);
        const dim3 grid((unsigned)blocks);
        if (odd) {
            const int ntx = (Xw + TG - 1) / TG, nty = (Xh + TG - 1) / TG;
            if (src_is_u8) hipLaunchKernelGGL(tta_transpose_kernel<unsigned char>, grid, dim3(256), 0, st, (const unsigned char*)src, src_hwc, swap_rb, out, packed, B, C, h, w, Xh, Xw, ntx, nty);
            else hipLaunchKernelGGL(tta_transpose_kernel<float>, grid, dim3(256), 0, st, (const float*)src, src_hwc, swap_rb, out, packed, B, C, h, w, Xh, Xw, ntx, nty);
        } else {
            const int nseg = (Xw + SEG - 1) / SEG;
            const bool vec = Xw % 4 == 0 && aligned16(out);
            if (src_is_u8 && vec) hipLaunchKernelGGL((tta_rows_kernel<unsigned char, true>), grid, dim3(256), 0, st, (const unsigned char*)src, src_hwc, swap_rb, out, packed, B, C, h, w, Xh, Xw, nseg);
            else if (src_is_u8) hipLaunchKernelGGL((tta_rows_kernel<unsigned char, false>), grid, dim3(256), 0, st, (const unsigned char*)src, src_hwc, swap_rb, out, packed, B, C, h, w, Xh, Xw, nseg);
            else if (vec) hipLaunchKernelGGL((tta_rows_kernel<float, true>), grid, dim3(256), 0, st, (const float*)src, src_hwc, swap_rb, out, packed, B, C, h, w, Xh, Xw, nseg);
            else hipLaunchKernelGGL((tta_rows_kernel<float, false>), grid, dim3(256), 0, st, (const float*)src, src_hwc, swap_rb, out, packed, B, C, h, w, Xh, Xw, nseg);
        }
    }
    return check_launch("tta_gather");
}

extern "C" int uf_tta_merge(const float* even, const int* ks_even, int ne, int Xh, int Xw, const float* odd, const int* ks_odd, int no, int Xoh, int Xow, void* out,
                            int out_is_u8, int out_hwc, int swap_rb, int clamp01, int B, int C, int h, int w, void* stream) {
    UF_REQUIRE(out && (ne <= 0 || (even && ks_even)) && (no <= 0 || (odd && ks_odd)), UF_ERR_NULL, "uf_tta_merge: null pointer");
    const int max_c = out_is_u8 ? MAX_C_U8 : MAX_C;
    UF_REQUIRE(C >= 1 && C <= max_c, UF_ERR_UNSUPPORTED, "uf_tta_merge: C=%d (1 ... %d channels for %s output)", C, max_c, out_is_u8 ? "u8" : "f32");
    UF_REQUIRE(!swap_rb || C >= 3, UF_ERR_UNSUPPORTED, "uf_tta_merge: swap_rb needs C >= 3, got C=%d", C);
    UF_REQUIRE(ne >= 0 && no >= 0 && ne <= 4 && no <= 4, UF_ERR_UNSUPPORTED, "uf_tta_merge: ne=%d no=%d (0 ... 4 members of each parity)", ne, no);
    const int n = ne + no;
    UF_REQUIRE(n == 1 || n == 2 || n == 4 || n == 8, UF_ERR_UNSUPPORTED, "uf_tta_merge: n=%d members (1, 2, 4 or 8)", n);
    if (const int rc = check_members("uf_tta_merge", "ks_even", ks_even, ne, 0)) return rc;
    if (const int rc = check_members("uf_tta_merge", "ks_odd", ks_odd, no, 1)) return rc;
    UF_REQUIRE(B > 0 && h > 0 && w > 0, UF_ERR_SHAPE, "uf_tta_merge: B=%d h=%d w=%d", B, h, w);
    UF_REQUIRE(ne == 0 || (Xh >= h && Xw >= w), UF_ERR_SHAPE, "uf_tta_merge: even canvas Xh=%d Xw=%d smaller than the member h=%d w=%d", Xh, Xw, h, w);
    UF_REQUIRE(no == 0 || (Xoh >= w && Xow >= h), UF_ERR_SHAPE, "uf_tta_merge: odd canvas Xh=%d Xw=%d smaller than the member h=%d w=%d", Xoh, Xow, w, h);
    const long long n_even = ne ? capped_product({ne, B, C, Xh, Xw}) : 0, n_odd = no ? capped_product({no, B, C, Xoh, Xow}) : 0, n_out = capped_product({B, C, h, w});
    const int ntx = (w - 1) / TM + 1, nty = (h - 1) / TM + 1;
    UF_REQUIRE(n_even < LIMIT31 && n_odd < LIMIT31 && n_out < LIMIT31 && capped_product({B, ntx, nty}) < LIMIT31, UF_ERR_SHAPE,
               "uf_tta_merge: %lld even and %lld odd canvas elements, B*C*h*w = %lld frame elements (2^31 stands for more), the limit is 2^31", n_even, n_odd, n_out);
    MergePlan p{};                                                    // the two lists merged in ascending k
    p.staged = no > 0;
    for (int j = 0, ie = 0, io = 0; j < n; ++j) {
        const bool take_odd = ie >= ne || (io < no && ks_odd[io] < ks_even[ie]);
        const int k = take_odd ? ks_odd[io] : ks_even[ie];
        const int fy = (0x36 >> k) & 1, fx = (0x6C >> k) & 1;          // flips_y, flips_x
        if (take_odd) {
            p.base[j] = (long long)io * B * C * Xoh * Xow + (long long)((Xoh - w) / 2) * Xow + (Xow - h) / 2;
            p.dy[j] = fy; p.dx[j] = fx; p.slot[j] = io++;
        } else {
            p.base[j] = (long long)ie * B * C * Xh * Xw + (long long)((Xh - h) / 2 + (fy ? h - 1 : 0)) * Xw + (Xw - w) / 2 + (fx ? w - 1 : 0);
            p.dy[j] = fy ? -Xw : Xw; p.dx[j] = fx ? -1 : 1; p.slot[j] = -1; ++ie;
        }
    }
    const dim3 grid((unsigned)((long long)B * ntx * nty));
    hipStream_t st = (hipStream_t)stream;
    {
        ScopedTimer tm("tta_merge", 0.0, (4.0 * n + (out_is_u8 ? 1.0 : 4.0)) * B * C * h * w, st);
#define UF_MERGE(U8, N) hipLaunchKernelGGL((tta_merge_kernel<U8, N>), grid, dim3(256), 0, st, even, Xh, Xw, odd, Xoh, Xow, p, 1.0f / (float)n, out, out_hwc, swap_rb, clamp01, B, C, h, w, ntx, nty)
        if (out_is_u8) { if (n == 8) UF_MERGE(true, 8); else if (n == 4) UF_MERGE(true, 4); else if (n == 2) UF_MERGE(true, 2); else UF_MERGE(true, 1); }
        else { if (n == 8) UF_MERGE(false, 8); else if (n == 4) UF_MERGE(false, 4); else if (n == 2) UF_MERGE(false, 2); else UF_MERGE(false, 1); }
#undef UF_MERGE
    }
    return check_launch("tta_merge");
}
