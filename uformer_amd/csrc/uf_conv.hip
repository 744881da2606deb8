// Dense convolutions of the UNet baseline (reference model.py:83-174) as implicit GEMMs on MFMA:
//   uf_conv3x3_fwd   3x3 stride 1 pad 1, Cin -> Cout, with the ConvBlock epilogues (bias, LeakyReLU, + conv11 branch, dgrad)
//   uf_conv1x1_fwd   1x1 (ConvBlock.conv11)
//   uf_conv4s2_fwd   4x4 stride 2 pad 1, Cin -> Cout (UNet.pool1..4; Downsample's uf_downsample_fwd is fixed at Cout = 2 Cin)
//   uf_conv1x1_nchw_fwd  ConvBlock1.conv11 (Cin = 3) straight from the NCHW image
//
// One workgroup computes a tile of TH x TW = 128 output pixels x 64 output channels.  For each chunk of 32 input channels it stages
// the tile's input pixels plus the halo in LDS once (f32 rows -> operand type T), then every tap reads its A fragments from LDS
// and streams its B fragments (the packed weight) from L2 straight into registers.  Four waves, each 32 pixels x 64 channels:
// 2 x 4 accumulators of 16 x 16.  Layouts: include/uformer_hip.h.
#include <algorithm>

#include "uf_internal.h"

namespace uf {
namespace {

constexpr int CV_BN = 64;       // output channels per workgroup
constexpr int CV_KC = 32;       // input channels per staged chunk = one MFMA k-step per tap
constexpr int CV_PIX = 128;     // output pixels per workgroup
constexpr int CV_THREADS = 256;

enum ConvEpi { CE_BIAS = 0, CE_LRELU = 1, CE_LRELU_ADD = 2, CE_DGRAD = 3 };
constexpr float LRELU_SLOPE = 0.01f;   // nn.LeakyReLU() default

template <int KS, int S, int TW> struct ConvGeo {
    static constexpr int TH = CV_PIX / TW;
    static constexpr int HH = (TH - 1) * S + KS;    // staged rows (with halo)
    static constexpr int HWD = (TW - 1) * S + KS;   // staged columns
};
// LDS pixel stride in elements: 32 channels + 16 bytes of padding (breaks the power-of-two stride between neighbouring pixels)
template <typename T> constexpr int lds_pix() { return CV_KC + 16 / (int)sizeof(T); }
template <typename T, int KS, int S, int TW> constexpr int conv_lds_bytes() {
    return ConvGeo<KS, S, TW>::HH * ConvGeo<KS, S, TW>::HWD * lds_pix<T>() * (int)sizeof(T);
}

struct ConvArgs {
    const float* x; int ld_x;
    const void* w; const float* bias;
    const float* aux; int ld_aux;
    float* out; int ld_o;
    int B, H, W, Ho, Wo, Cin, Cout, Cin_p;
    int pad, epi, accumulate;
    int tiles_x, tiles_y, nblk;
};

template <typename T, int KS, int S, int TW>
__global__ __launch_bounds__(CV_THREADS) void conv_igemm_kernel(ConvArgs a) {
    using G = ConvGeo<KS, S, TW>;
    constexpr int PIX = lds_pix<T>();
    extern __shared__ __align__(16) unsigned char cv_smem[];
    T* sx = reinterpret_cast<T*>(cv_smem);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nb = blockIdx.x % a.nblk;
    int t = blockIdx.x / a.nblk;
    const int tx = t % a.tiles_x; t /= a.tiles_x;
    const int ty = t % a.tiles_y;
    const int b = t / a.tiles_y;
    const int oy0 = ty * G::TH, ox0 = tx * TW, n0 = nb * CV_BN;
    const int iy0 = oy0 * S - a.pad, ix0 = ox0 * S - a.pad;

    // A rows of this lane: pixel m = 32 wave + 16 mi + (lane & 15); k-slots 8g..8g+7 of the chunk, g = lane >> 4
    const int g = lane >> 4, r16 = lane & 15;
    int abase[2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
        const int m = 32 * wave + 16 * mi + r16;
        abase[mi] = ((m / TW) * S * G::HWD + (m % TW) * S) * PIX + 8 * g;
    }
    const int Ktot = KS * KS * a.Cin_p;
    const T* wrow[4];
#pragma unroll
    for (int nj = 0; nj < 4; ++nj) wrow[nj] = reinterpret_cast<const T*>(a.w) + (size_t)(n0 + 16 * nj + r16) * Ktot + 8 * g;

    f32x4 acc[2][4];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int nj = 0; nj < 4; ++nj) acc[mi][nj] = f32x4{0, 0, 0, 0};

    const size_t img_row0 = (size_t)b * a.H;
    for (int c0 = 0; c0 < a.Cin_p; c0 += CV_KC) {
        // ---- stage the halo tile of channels [c0, c0 + 32): quads of 4 channels, zero outside the image and beyond Cin
        for (int i = tid; i < G::HH * G::HWD * (CV_KC / 4); i += CV_THREADS) {
            const int q = i & 7, p = i >> 3;
            const int hy = p / G::HWD, hx = p - hy * G::HWD;
            const int iy = iy0 + hy, ix = ix0 + hx, c = c0 + 4 * q;
            f32x4 v = f32x4{0, 0, 0, 0};
            if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W && c < a.Cin)
                v = *reinterpret_cast<const f32x4*>(a.x + ((img_row0 + iy) * a.W + ix) * (size_t)a.ld_x + c);
            store4(sx + p * PIX + 4 * q, v);
        }
        __syncthreads();
        // ---- all taps of the chunk
#pragma unroll 3
        for (int tap = 0; tap < KS * KS; ++tap) {
            const int ky = tap / KS, kx = tap - ky * KS;
            const int koff = tap * a.Cin_p + c0;
            Frag<T> bf[4];
#pragma unroll
            for (int nj = 0; nj < 4; ++nj) load_frag(bf[nj], wrow[nj] + koff);
            const int toff = (ky * G::HWD + kx) * PIX;
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) {
                Frag<T> af;
                load_frag(af, sx + abase[mi] + toff);
#pragma unroll
                for (int nj = 0; nj < 4; ++nj) mma16(acc[mi][nj], af, bf[nj]);
            }
        }
        __syncthreads();
    }

    // ---- epilogue: D row = 4 (lane >> 4) + reg, column = lane & 15
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = 32 * wave + 16 * mi + 4 * g + r;
            const int oy = oy0 + m / TW, ox = ox0 + m % TW;
            if (oy >= a.Ho || ox >= a.Wo) continue;
            const size_t row = ((size_t)b * a.Ho + oy) * a.Wo + ox;
#pragma unroll
            for (int nj = 0; nj < 4; ++nj) {
                const int n = n0 + 16 * nj + r16;
                if (n >= a.Cout) continue;
                float v = acc[mi][nj][r];
                float* o = a.out + row * a.ld_o + n;
                if (a.epi == CE_DGRAD) {
                    v *= a.aux[row * a.ld_aux + n] > 0.0f ? 1.0f : LRELU_SLOPE;
                    if (a.accumulate) v += *o;
                } else {
                    v += a.bias[n];
                    if (a.epi != CE_BIAS) v = v > 0.0f ? v : v * LRELU_SLOPE;
                    if (a.epi == CE_LRELU_ADD) v += a.aux[row * a.ld_aux + n];
                    if (a.accumulate) v += *o;
                }
                *o = v;
            }
        }
    }
}

template <typename T, int KS, int S, int TW>
int launch_tw(const ConvArgs& a0, hipStream_t st) {
    using G = ConvGeo<KS, S, TW>;
    ConvArgs a = a0;
    a.tiles_x = (a.Wo + TW - 1) / TW;
    a.tiles_y = (a.Ho + G::TH - 1) / G::TH;
    a.nblk = (a.Cout + CV_BN - 1) / CV_BN;
    const long long blocks = (long long)a.tiles_x * a.tiles_y * a.B * a.nblk;
    UF_REQUIRE(blocks < 0x7fffffffLL, UF_ERR_SHAPE, "conv: grid of %lld workgroups too large", blocks);
    constexpr int lds = conv_lds_bytes<T, KS, S, TW>();
    if (lds > 65536) {
        static bool done[64] = {};
        const int rc = ensure_dynamic_lds((const void*)conv_igemm_kernel<T, KS, S, TW>, lds, done, "conv");
        if (rc) return rc;
    }
    hipLaunchKernelGGL((conv_igemm_kernel<T, KS, S, TW>), dim3((unsigned)blocks), dim3(CV_THREADS), lds, st, a);
    return check_launch("conv_igemm");
}

// tile width: the widest of 16 / 8 / 4 that the output map fills (the bottleneck of a 64x64 input is 4x4)
template <typename T, int KS, int S>
int launch_conv_t(const ConvArgs& a, hipStream_t st) {
    if (a.Wo >= 16) return launch_tw<T, KS, S, 16>(a, st);
    if (a.Wo >= 8) return launch_tw<T, KS, S, 8>(a, st);
    return launch_tw<T, KS, S, 4>(a, st);
}

int check_common(const char* what, const float* x, int ld_x, const void* w, float* out, int ld_o, int B, int H, int W, int Cin, int Cout, uf_dtype dtype) {
    UF_REQUIRE(x && w && out, UF_ERR_NULL, "%s: null pointer", what);
    UF_REQUIRE(dtype_ok(dtype), UF_ERR_UNSUPPORTED, "%s: dtype %d", what, (int)dtype);
    UF_REQUIRE(B > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, UF_ERR_SHAPE, "%s: B=%d H=%d W=%d Cin=%d Cout=%d", what, B, H, W, Cin, Cout);
    UF_REQUIRE(Cin % 4 == 0 && ld_x >= Cin && ld_x % 4 == 0 && ld_o >= Cout, UF_ERR_SHAPE,
               "%s: Cin=%d must be a multiple of 4, ld_x=%d a multiple of 4 and >= Cin, ld_o=%d >= Cout=%d", what, Cin, ld_x, ld_o, Cout);
    UF_REQUIRE(((uintptr_t)x % 16) == 0 && ((uintptr_t)w % 16) == 0, UF_ERR_ALIGN, "%s: x and w must be 16-byte aligned", what);
    UF_REQUIRE((long long)B * H * W * ld_x < (1LL << 40), UF_ERR_SHAPE, "%s: tensor too large", what);
    return UF_OK;
}

int run_conv(int KS, ConvArgs a, uf_dtype dtype, hipStream_t st) {
    a.Cin_p = (a.Cin + CV_KC - 1) / CV_KC * CV_KC;
    const double flops = 2.0 * a.B * a.Ho * a.Wo * (double)a.Cout * a.Cin * KS * KS;
    const double bytes = 4.0 * ((double)a.B * a.H * a.W * a.Cin + (double)a.B * a.Ho * a.Wo * a.Cout) +
                         (double)dtype_size(dtype) * a.Cout * a.Cin * KS * KS;
    const char* name = KS == 3 ? "conv3x3" : (KS == 1 ? "conv1x1" : "conv4s2");
    ScopedTimer tm(name, flops, bytes, st);
    int rc = UF_OK;
    if (KS == 3) { UF_DISPATCH(dtype, TT, rc = (launch_conv_t<TT, 3, 1>(a, st))); }
    else if (KS == 1) { UF_DISPATCH(dtype, TT, rc = (launch_conv_t<TT, 1, 1>(a, st))); }
    else { UF_DISPATCH(dtype, TT, rc = (launch_conv_t<TT, 4, 2>(a, st))); }
    return rc;
}

// ConvBlock1.conv11: 1x1 conv of the NCHW image (Cin <= 4) into token rows; one thread per output element
__global__ void conv1x1_nchw_kernel(const float* __restrict__ img, const float* __restrict__ w, const float* __restrict__ bias,
                                    float* __restrict__ out, int ld_o, int B, int Cin, int HW, int Cout) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B * HW * Cout) return;
    const int co = (int)(i % Cout);
    const long long pix = i / Cout;
    const int b = (int)(pix / HW), p = (int)(pix - (long long)b * HW);
    float v = bias[co];
    for (int c = 0; c < Cin; ++c) v = fmaf(w[co * Cin + c], img[((size_t)b * Cin + c) * HW + p], v);
    out[pix * ld_o + co] = v;
}

}  // namespace
}  // namespace uf

using namespace uf;

extern "C" size_t uf_conv_packed_elems(int Cout, int Cin, int k) {
    if (Cout <= 0 || Cin <= 0 || k <= 0) return 0;
    return (size_t)((Cout + CV_BN - 1) / CV_BN * CV_BN) * k * k * ((Cin + CV_KC - 1) / CV_KC * CV_KC);
}

extern "C" int uf_conv3x3_fwd(const float* x, int ld_x, const void* w_pk, const float* bias, const float* aux, int ld_aux, float* out, int ld_o,
                              int B, int H, int W, int Cin, int Cout, int epilogue, int accumulate, uf_dtype dtype, void* stream) {
    int rc = check_common("uf_conv3x3_fwd", x, ld_x, w_pk, out, ld_o, B, H, W, Cin, Cout, dtype);
    if (rc) return rc;
    UF_REQUIRE(epilogue >= CE_BIAS && epilogue <= CE_DGRAD, UF_ERR_UNSUPPORTED, "uf_conv3x3_fwd: epilogue %d", epilogue);
    UF_REQUIRE(epilogue == CE_DGRAD || bias, UF_ERR_NULL, "uf_conv3x3_fwd: null bias");
    UF_REQUIRE(epilogue < CE_LRELU_ADD || (aux && ld_aux >= Cout), UF_ERR_NULL, "uf_conv3x3_fwd: epilogue %d needs aux rows of >= Cout channels", epilogue);
    ConvArgs a{};
    a.x = x; a.ld_x = ld_x; a.w = w_pk; a.bias = bias; a.aux = aux; a.ld_aux = ld_aux; a.out = out; a.ld_o = ld_o;
    a.B = B; a.H = H; a.W = W; a.Ho = H; a.Wo = W; a.Cin = Cin; a.Cout = Cout; a.pad = 1; a.epi = epilogue; a.accumulate = accumulate ? 1 : 0;
    return run_conv(3, a, dtype, (hipStream_t)stream);
}

extern "C" int uf_conv1x1_fwd(const float* x, int ld_x, const void* w_pk, const float* bias, float* out, int ld_o, int B, int H, int W,
                              int Cin, int Cout, uf_dtype dtype, void* stream) {
    int rc = check_common("uf_conv1x1_fwd", x, ld_x, w_pk, out, ld_o, B, H, W, Cin, Cout, dtype);
    if (rc) return rc;
    UF_REQUIRE(bias, UF_ERR_NULL, "uf_conv1x1_fwd: null bias");
    ConvArgs a{};
    a.x = x; a.ld_x = ld_x; a.w = w_pk; a.bias = bias; a.out = out; a.ld_o = ld_o;
    a.B = B; a.H = H; a.W = W; a.Ho = H; a.Wo = W; a.Cin = Cin; a.Cout = Cout; a.pad = 0; a.epi = CE_BIAS;
    return run_conv(1, a, dtype, (hipStream_t)stream);
}

extern "C" int uf_conv4s2_fwd(const float* x, int ld_x, const void* w_pk, const float* bias, float* out, int ld_o, int B, int H, int W,
                              int Cin, int Cout, uf_dtype dtype, void* stream) {
    int rc = check_common("uf_conv4s2_fwd", x, ld_x, w_pk, out, ld_o, B, H, W, Cin, Cout, dtype);
    if (rc) return rc;
    UF_REQUIRE(bias, UF_ERR_NULL, "uf_conv4s2_fwd: null bias");
    UF_REQUIRE(H % 2 == 0 && W % 2 == 0, UF_ERR_SHAPE, "uf_conv4s2_fwd: H=%d W=%d must be even", H, W);
    ConvArgs a{};
    a.x = x; a.ld_x = ld_x; a.w = w_pk; a.bias = bias; a.out = out; a.ld_o = ld_o;
    a.B = B; a.H = H; a.W = W; a.Ho = H / 2; a.Wo = W / 2; a.Cin = Cin; a.Cout = Cout; a.pad = 1; a.epi = CE_BIAS;
    return run_conv(4, a, dtype, (hipStream_t)stream);
}

extern "C" int uf_conv1x1_nchw_fwd(const float* img, const float* w, const float* bias, float* out, int ld_o, int B, int Cin, int H, int W,
                                   int Cout, void* stream) {
    UF_REQUIRE(img && w && bias && out, UF_ERR_NULL, "uf_conv1x1_nchw_fwd: null pointer");
    UF_REQUIRE(B > 0 && H > 0 && W > 0 && Cin > 0 && Cin <= 4 && Cout > 0 && ld_o >= Cout, UF_ERR_SHAPE,
               "uf_conv1x1_nchw_fwd: B=%d Cin=%d (<= 4) H=%d W=%d Cout=%d ld_o=%d", B, Cin, H, W, Cout, ld_o);
    const long long n = (long long)B * H * W * Cout;
    UF_REQUIRE(n / 256 < 0x7fffffffLL, UF_ERR_SHAPE, "uf_conv1x1_nchw_fwd: too large");
    hipStream_t st = (hipStream_t)stream;
    ScopedTimer tm("conv1x1_nchw", 2.0 * n * Cin, 4.0 * ((double)B * H * W * Cin + n), st);
    hipLaunchKernelGGL(conv1x1_nchw_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, img, w, bias, out, ld_o, B, Cin, H * W, Cout);
    return check_launch("conv1x1_nchw");
}

// ------------------------------------------------------------------------------------------
// whole UNet (reference model.py:128-174): one call per forward, f32 activation rows throughout
// ------------------------------------------------------------------------------------------
namespace {
struct UnetPlan {
    int C[9], lvl[9];         // ConvBlock i+1: output width and resolution level (H >> lvl, W >> lvl)
    size_t M[5];              // pixels per level
    size_t off_D[4];          // concat buffers of ConvBlock6..9 (levels 3,2,1,0): rows of 2 C, [0,C) = upv*, [C,2C) = encoder skip
    size_t off_T, off_R, off_Y;   // first conv's output, conv11 branch, pool / decoder output
    size_t total;
};

int make_unet_plan(UnetPlan& pl, const uf_unet_desc* d, int B, int H, int W) {
    UF_REQUIRE(d, UF_ERR_NULL, "uf_unet: desc is null");
    UF_REQUIRE(B > 0, UF_ERR_SHAPE, "uf_unet: B=%d", B);
    UF_REQUIRE(H > 0 && H % 16 == 0, UF_ERR_SHAPE, "uf_unet: H=%d must be a positive multiple of 16 (4 stride-2 convolutions)", H);
    UF_REQUIRE(W > 0 && W % 16 == 0, UF_ERR_SHAPE, "uf_unet: W=%d must be a positive multiple of 16 (4 stride-2 convolutions)", W);
    UF_REQUIRE(d->dim >= 4 && d->dim % 4 == 0, UF_ERR_SHAPE, "uf_unet: dim=%d must be a multiple of 4", d->dim);
    const int mult[9] = {1, 2, 4, 8, 16, 8, 4, 2, 1};
    const int lvl[9] = {0, 1, 2, 3, 4, 3, 2, 1, 0};
    for (int i = 0; i < 9; ++i) { pl.C[i] = d->dim * mult[i]; pl.lvl[i] = lvl[i]; }
    for (int l = 0; l < 5; ++l) pl.M[l] = (size_t)B * (H >> l) * (W >> l);
    size_t off = 0, big = 0;
    for (int k = 0; k < 4; ++k) {
        pl.off_D[k] = off;
        off += align_up(pl.M[3 - k] * 2 * pl.C[5 + k] * sizeof(float), 256);
    }
    for (int i = 0; i < 9; ++i) big = std::max(big, pl.M[lvl[i]] * pl.C[i] * sizeof(float));
    big = std::max(big, pl.M[1] * pl.C[0] * sizeof(float));
    big = align_up(big, 256);
    pl.off_T = off; off += big;
    pl.off_R = off; off += big;
    pl.off_Y = off; off += big;
    pl.total = off;
    return UF_OK;
}
}  // namespace

extern "C" size_t uf_unet_workspace_bytes(const uf_unet_desc* d, int B, int H, int W, uf_dtype dtype) {
    if (!dtype_ok(dtype)) { set_error("uf_unet_workspace_bytes: dtype %d", (int)dtype); return 0; }
    UnetPlan pl;
    if (make_unet_plan(pl, d, B, H, W)) return 0;
    return pl.total;
}

extern "C" int uf_unet_fwd(const uf_unet_desc* d, const float* img, float* out, int B, int H, int W, uf_dtype dtype, void* ws,
                           size_t ws_bytes, void* stream) {
    UnetPlan pl;
    int rc = make_unet_plan(pl, d, B, H, W);
    if (rc) return rc;
    UF_REQUIRE(img && out && ws, UF_ERR_NULL, "uf_unet_fwd: null pointer");
    UF_REQUIRE(ws_bytes >= pl.total, UF_ERR_WORKSPACE, "uf_unet_fwd: workspace %zu < %zu bytes", ws_bytes, pl.total);
    UF_REQUIRE(((uintptr_t)ws % 256) == 0, UF_ERR_ALIGN, "uf_unet_fwd: workspace must be 256-byte aligned");
    char* base = (char*)ws;
    float* D[4];
    for (int k = 0; k < 4; ++k) D[k] = (float*)(base + pl.off_D[k]);
    float* T1 = (float*)(base + pl.off_T);
    float* R = (float*)(base + pl.off_R);
    float* Y = (float*)(base + pl.off_Y);
    const int e = d->dim;
    // ConvBlock1 (3 -> dim) on the image: block.0 = InputProj's conv3x3 + LeakyReLU, conv11 from the NCHW planes, block.2 + LeakyReLU + conv11
    // written into the skip half of ConvBlock9's concat buffer
    rc = uf_input_proj_fwd(img, d->in_w27, d->in_b, T1, e, B, 3, H, W, e, stream);
    if (rc) return rc;
    rc = uf_conv1x1_nchw_fwd(img, d->c11_w1, d->c11_b1, R, e, B, 3, H, W, e, stream);
    if (rc) return rc;
    rc = uf_conv3x3_fwd(T1, e, d->w2[0], d->b2[0], R, e, D[3] + e, 2 * e, B, H, W, e, e, CE_LRELU_ADD, 0, dtype, stream);
    if (rc) return rc;
    // ConvBlock i+1 (i >= 1) at (h, w): block.0 + LeakyReLU -> T1, conv11 -> R, block.2 + LeakyReLU + R -> dst
    auto conv_block = [&](int i, const float* in, int ld_in, int cin, int h, int w, float* dst, int ld_dst) -> int {
        const int C = pl.C[i];
        int r = uf_conv3x3_fwd(in, ld_in, d->w0[i], d->b0[i], nullptr, 0, T1, C, B, h, w, cin, C, CE_LRELU, 0, dtype, stream);
        if (r) return r;
        r = uf_conv1x1_fwd(in, ld_in, d->w11[i], d->b11[i], R, C, B, h, w, cin, C, dtype, stream);
        if (r) return r;
        return uf_conv3x3_fwd(T1, C, d->w2[i], d->b2[i], R, C, dst, ld_dst, B, h, w, C, C, CE_LRELU_ADD, 0, dtype, stream);
    };
    // encoder: pool k (k4 s2 p1, C -> C) of ConvBlock k+1's output (the skip half of its concat buffer) into Y, then ConvBlock k+2;
    // ConvBlock2..4 write into the skip half of their decoder concat buffer, ConvBlock5 into Y
    for (int k = 0; k < 4; ++k) {
        const int i = k + 1, cin = pl.C[k], C = pl.C[i], h = H >> i, w = W >> i;
        const float* skip = D[3 - k] + cin;
        rc = uf_conv4s2_fwd(skip, 2 * cin, d->pool_w[k], d->pool_b[k], Y, cin, B, 2 * h, 2 * w, cin, cin, dtype, stream);
        if (rc) return rc;
        rc = i < 4 ? conv_block(i, Y, cin, cin, h, w, D[3 - i] + C, 2 * C) : conv_block(i, Y, cin, cin, h, w, Y, C);
        if (rc) return rc;
    }
    // decoder: upv (ConvTranspose2d k2 s2) of Y into channels [0, C) of the concat buffer, then ConvBlock6..9 into Y
    for (int k = 0; k < 4; ++k) {
        const int i = 5 + k, C = pl.C[i], cin = pl.C[i - 1], h = H >> pl.lvl[i], w = W >> pl.lvl[i];
        rc = uf_upsample_fwd(Y, cin, d->up_w[k], d->up_b[k], D[k], 2 * C, B, h / 2, w / 2, cin, C, dtype, stream);
        if (rc) return rc;
        rc = conv_block(i, D[k], 2 * C, 2 * C, h, w, Y, C);
        if (rc) return rc;
    }
    // conv10 + the global residual x + conv10 (OutputProj's kernel, model.py:171-172)
    return uf_output_proj_fwd(Y, e, d->out_w, d->out_b, img, out, B, H, W, e, 1, stream);
}
