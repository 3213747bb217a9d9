// Image generator (include/xlxmert_hip.h, section "image generator"): the kernels of the frozen SPADE decoder, NHWC activations.
//   conv_mfma_kernel      3x3 / 1x1 convolution as an implicit GEMM on v_mfma_f32_32x32x16_bf16: a workgroup owns 8 x 32 output pixels x
//                         all of Cout, stages the haloed input tile in LDS once and walks taps x Cin/16 steps reading the input fragments
//                         at shifted LDS addresses (no im2col buffer).  The WEIGHTS are the A operand (rows = output channels), the
//                         pixels the B operand (columns = the 32 pixels of one tile row): an accumulator lane then holds, for ONE pixel,
//                         groups of 4 consecutive output channels -- gamma and beta of the SPADE epilogue meet in the same lane, and a
//                         store is 8 bytes of 4 channels.
//   conv_generic_kernel   one thread per output element, plain FMA: fp32, grouped, Cout = 3, odd channel counts; same epilogues.
//   instnorm_*            per-(image, channel) mean / rstd in two stages of fixed order.
//   resize / torgb / normal planes: one thread per output element.
#include "common.h"

namespace xl {

struct ConvArgs {
    const void* x; const void* w; const float* bias; void* y; const void* aux;
    const float* mean; const float* rstd; const float* noise;
    float noise_w, slope;
    int B, H, W, Cin, Cout, ks, groups, ldx, ldy, ldaux, epi, tiles_x, tiles_y;
};

__device__ __forceinline__ float lrelu(float t, float s) { return t >= 0.f ? t : s * t; }

// ---------------------------------------------------------------- generic convolution
template <typename T>
__device__ __forceinline__ float conv_at(const ConvArgs& a, int b, int y, int x, int co) {
    const int Cg = a.Cin / a.groups, g = co / (a.Cout / a.groups), pad = a.ks >> 1;
    const T* __restrict__ xin = (const T*)a.x;
    const T* __restrict__ w = (const T*)a.w;
    float acc = 0.f;
    for (int kh = 0; kh < a.ks; ++kh) {
        const int iy = y + kh - pad;
        if (iy < 0 || iy >= a.H) continue;
        for (int kw = 0; kw < a.ks; ++kw) {
            const int ix = x + kw - pad;
            if (ix < 0 || ix >= a.W) continue;
            const T* xp = xin + (((int64_t)b * a.H + iy) * a.W + ix) * a.ldx + g * Cg;
            const T* wp = w + ((int64_t)(kh * a.ks + kw) * a.Cout + co) * Cg;
            for (int ci = 0; ci < Cg; ++ci) acc = fmaf(Elem<T>::ld(xp + ci), Elem<T>::ld(wp + ci), acc);
        }
    }
    return a.bias != nullptr ? acc + a.bias[co] : acc;
}

template <typename T>
__global__ __launch_bounds__(256) void conv_generic_kernel(ConvArgs a) {
    const int Cy = a.epi == XL_CONV_SPADE ? a.Cout / 2 : a.Cout;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t HW = (int64_t)a.H * a.W;
    if (t >= (int64_t)a.B * HW * Cy) return;
    const int c = (int)(t % Cy);
    const int64_t pix = t / Cy;                 // b*HW + p
    const int b = (int)(pix / HW);
    const int p = (int)(pix - (int64_t)b * HW);
    const int y = p / a.W, x = p - y * a.W;
    float v = conv_at<T>(a, b, y, x, c);
    if (a.epi == XL_CONV_RELU) {
        v = fmaxf(v, 0.f);
    } else if (a.epi == XL_CONV_ADD) {
        v += Elem<T>::ld((const T*)a.aux + pix * a.ldaux + c);
    } else if (a.epi == XL_CONV_SPADE) {
        const float beta = conv_at<T>(a, b, y, x, c + Cy);
        const float xn = (Elem<T>::ld((const T*)a.aux + pix * a.ldaux + c) - a.mean[b * Cy + c]) * a.rstd[b * Cy + c];
        float tt = xn * (1.f + v) + beta;
        if (a.noise != nullptr) tt += a.noise_w * a.noise[pix];
        v = lrelu(tt, a.slope);
    }
    Elem<T>::st((T*)a.y + pix * a.ldy + c, v);
}

// ---------------------------------------------------------------- MFMA convolution (bf16)
constexpr int CT_H = 8, CT_W = 32;          // output pixels of a workgroup: 4 waves x 2 tile rows of 32 pixels
constexpr int CONV_LDS_MAX = 160 * 1024;

__device__ __forceinline__ f32x16_t conv_mfma32(bf16x8_t a, bf16x8_t b, f32x16_t c) {
    typedef __attribute__((ext_vector_type(8))) __bf16 v8_t;
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8_t, a), __builtin_bit_cast(v8_t, b), c, 0, 0, 0);
}

// LDS image: (CT_H + 2 pad) x (CT_W + 2 pad) pixels, Cin bf16 each, pixel stride Cin*2 + 16 bytes -- an ODD number of 16-byte slots
// (Cin % 16 == 0), so the 16 lanes that a ds_read_b128 serves together (16 consecutive pixels, same k offset) hit 16 different slots.
template <int MT>
__global__ __launch_bounds__(256) void conv_mfma_kernel(ConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t conv_smem[];
    const int pad = a.ks >> 1;
    const int LW = CT_W + 2 * pad, LH = CT_H + 2 * pad;
    const int PS = a.Cin * 2 + 16;
    const int vpp = a.Cin >> 3;
    int tile = blockIdx.x;
    const int tx = tile % a.tiles_x; tile /= a.tiles_x;
    const int ty = tile % a.tiles_y;
    const int b = tile / a.tiles_y;
    const int x0 = tx * CT_W, y0 = ty * CT_H;
    const int64_t HW = (int64_t)a.H * a.W;
    const bf16_t* __restrict__ xb = (const bf16_t*)a.x + (int64_t)b * HW * a.ldx;
    for (int i = threadIdx.x; i < LH * LW * vpp; i += 256) {
        const int pix = i / vpp, v = i - pix * vpp;
        const int ly = pix / LW, lx = pix - ly * LW;
        const int gy = y0 + ly - pad, gx = x0 + lx - pad;
        uint4 val = make_uint4(0u, 0u, 0u, 0u);                 // outside the image: the zero padding
        if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) val = *reinterpret_cast<const uint4*>(xb + ((int64_t)gy * a.W + gx) * a.ldx + v * 8);
        *reinterpret_cast<uint4*>(conv_smem + pix * PS + v * 16) = val;
    }
    __syncthreads();

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    f32x16_t acc[MT][2];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[mt][nt][q] = 0.f;
    const bf16_t* __restrict__ wl = (const bf16_t*)a.w + (int64_t)r * a.Cin + 8 * h;        // output channel r of M tile 0, this lane's k
    const int kcn = a.Cin >> 4, taps = a.ks * a.ks;
    for (int tap = 0; tap < taps; ++tap) {
        const int kh = tap / a.ks, kw = tap - kh * a.ks;
        const uint8_t* s0 = conv_smem + ((2 * wave + kh) * LW + r + kw) * PS + 16 * h;       // tile row 2*wave; row 2*wave + 1 is LW*PS further
        const bf16_t* wt = wl + (int64_t)tap * a.Cout * a.Cin;
        for (int kc = 0; kc < kcn; ++kc) {
            const bf16x8_t b0 = *reinterpret_cast<const bf16x8_t*>(s0 + kc * 32);
            const bf16x8_t b1 = *reinterpret_cast<const bf16x8_t*>(s0 + LW * PS + kc * 32);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const bf16x8_t af = *reinterpret_cast<const bf16x8_t*>(wt + (int64_t)mt * 32 * a.Cin + kc * 16);
                acc[mt][0] = conv_mfma32(af, b0, acc[mt][0]);
                acc[mt][1] = conv_mfma32(af, b1, acc[mt][1]);
            }
        }
    }

    // accumulator register 4q + j of M tile mt: output channel mt*32 + 8q + 4h + j, pixel (tile row 2*wave + nt, column r)
    constexpr int C = 16 * MT;                  // SPADE: Cout = 32 MT = 2C
    const int gx = x0 + r;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int gy = y0 + 2 * wave + nt;
        if (gy >= a.H || gx >= a.W) continue;
        const int64_t pix = (int64_t)b * HW + (int64_t)gy * a.W + gx;
        if (a.epi == XL_CONV_SPADE) {
            const float nz = a.noise != nullptr ? a.noise_w * a.noise[pix] : 0.f;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (mt * 32 + 8 * q >= C) continue;                     // (static: the beta half is read below, not walked)
                    const int co = mt * 32 + 8 * q + 4 * h;
                    const float4 gb = *reinterpret_cast<const float4*>(a.bias + co);
                    const float4 bb = *reinterpret_cast<const float4*>(a.bias + C + co);
                    const float4 mu = *reinterpret_cast<const float4*>(a.mean + b * C + co);
                    const float4 rs = *reinterpret_cast<const float4*>(a.rstd + b * C + co);
                    const uint2 xa = *reinterpret_cast<const uint2*>((const bf16_t*)a.aux + pix * a.ldaux + co);
                    const float xv[4] = {__uint_as_float(xa.x << 16), __uint_as_float(xa.x & 0xffff0000u), __uint_as_float(xa.y << 16),
                                         __uint_as_float(xa.y & 0xffff0000u)};
                    const float gbv[4] = {gb.x, gb.y, gb.z, gb.w}, bbv[4] = {bb.x, bb.y, bb.z, bb.w};
                    const float muv[4] = {mu.x, mu.y, mu.z, mu.w}, rsv[4] = {rs.x, rs.y, rs.z, rs.w};
                    constexpr int DF = 8 * MT;                              // beta = the flat accumulator index + C/2
                    float o[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int f = mt * 16 + 4 * q + j + DF;
                        const float gamma = acc[mt][nt][4 * q + j] + gbv[j];
                        const float beta = acc[f / 16 < MT ? f / 16 : 0][nt][f % 16] + bbv[j];      // (the clamp only serves the skipped iterations)
                        o[j] = lrelu((xv[j] - muv[j]) * rsv[j] * (1.f + gamma) + beta + nz, a.slope);
                    }
                    *reinterpret_cast<uint2*>((bf16_t*)a.y + pix * a.ldy + co) = make_uint2(pack2bf(o[0], o[1]), pack2bf(o[2], o[3]));
                }
        } else {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int co = mt * 32 + 8 * q + 4 * h;
                    float o[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[j] = acc[mt][nt][4 * q + j];
                    if (a.bias != nullptr) {
                        const float4 bv = *reinterpret_cast<const float4*>(a.bias + co);
                        o[0] += bv.x; o[1] += bv.y; o[2] += bv.z; o[3] += bv.w;
                    }
                    if (a.epi == XL_CONV_RELU) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) o[j] = fmaxf(o[j], 0.f);
                    } else if (a.epi == XL_CONV_ADD) {
                        const uint2 xa = *reinterpret_cast<const uint2*>((const bf16_t*)a.aux + pix * a.ldaux + co);
                        o[0] += __uint_as_float(xa.x << 16); o[1] += __uint_as_float(xa.x & 0xffff0000u);
                        o[2] += __uint_as_float(xa.y << 16); o[3] += __uint_as_float(xa.y & 0xffff0000u);
                    }
                    *reinterpret_cast<uint2*>((bf16_t*)a.y + pix * a.ldy + co) = make_uint2(pack2bf(o[0], o[1]), pack2bf(o[2], o[3]));
                }
        }
    }
}

template <int MT>
static hipError_t launch_conv_mfma(const ConvArgs& a, int lds, hipStream_t st) {
    hipError_t e = hipSuccess;
    static bool attr = false;
    if (!attr) { e = hipFuncSetAttribute((const void*)conv_mfma_kernel<MT>, hipFuncAttributeMaxDynamicSharedMemorySize, CONV_LDS_MAX); attr = true; }
    hipLaunchKernelGGL(conv_mfma_kernel<MT>, dim3((unsigned)(a.B * a.tiles_y * a.tiles_x)), dim3(256), lds, st, a);
    return e;
}

// ---------------------------------------------------------------- instance-norm statistics
// stage 1: block (chunk j, image b).  ctile = min(C, 256) channels side by side, 256 / ctile pixel lanes; sums of (x - K) and
// (x - K)^2 with K = the chunk's first pixel of that channel; the pixel lanes are added in lane order by lane 0.
template <typename T>
__global__ __launch_bounds__(256) void instnorm_stage1_kernel(const T* __restrict__ x, float* __restrict__ ws, int HW, int C, int ld, int nchunks) {
    __shared__ float s1[256], s2[256];
    const int j = blockIdx.x, b = blockIdx.y;
    const int p0 = j * XL_INSTNORM_CHUNK, p1 = min(HW, p0 + XL_INSTNORM_CHUNK);
    const int ctile = min(C, 256), np = 256 / ctile;
    const int tc = threadIdx.x % ctile, tp = threadIdx.x / ctile;
    const T* __restrict__ xb = x + (int64_t)b * HW * ld;
    for (int cbase = 0; cbase < C; cbase += ctile) {
        const int c = cbase + tc;
        const bool on = tp < np && c < C;
        float a1 = 0.f, a2 = 0.f, K = 0.f;
        if (on) {
            K = Elem<T>::ld(xb + (int64_t)p0 * ld + c);
            for (int p = p0 + tp; p < p1; p += np) {
                const float d = Elem<T>::ld(xb + (int64_t)p * ld + c) - K;
                a1 += d;
                a2 = fmaf(d, d, a2);
            }
        }
        s1[threadIdx.x] = a1;
        s2[threadIdx.x] = a2;
        __syncthreads();
        if (on && tp == 0) {
            float t1 = 0.f, t2 = 0.f;
            for (int l = 0; l < np; ++l) { t1 += s1[l * ctile + tc]; t2 += s2[l * ctile + tc]; }
            const float n = (float)(p1 - p0);
            const float dm = t1 / n;
            float* o = ws + (((int64_t)b * nchunks + j) * C + c) * 2;
            o[0] = K + dm;
            o[1] = fmaxf(t2 - t1 * dm, 0.f);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void instnorm_stage2_kernel(const float* __restrict__ ws, float* __restrict__ mean, float* __restrict__ rstd,
                                                              int B, int HW, int C, int nchunks, float eps) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * C) return;
    const int b = i / C, c = i - b * C;
    float n = 0.f, m = 0.f, M2 = 0.f;
    for (int j = 0; j < nchunks; ++j) {
        const float* o = ws + (((int64_t)b * nchunks + j) * C + c) * 2;
        const float nj = (float)(min(HW, (j + 1) * XL_INSTNORM_CHUNK) - j * XL_INSTNORM_CHUNK);
        const float d = o[0] - m, nn = n + nj;
        m += d * (nj / nn);
        M2 += o[1] + d * d * (n * nj / nn);
        n = nn;
    }
    mean[i] = m;
    rstd[i] = 1.0f / sqrtf(M2 / n + eps);
}

// ---------------------------------------------------------------- bilinear resize (align_corners = False)
struct Tap { int i0, i1; float w0, w1; };
__device__ __forceinline__ Tap bilinear_tap(int dst, int in, int out) {
    const float scale = (float)in / (float)out;
    const float src = fmaxf(((float)dst + 0.5f) * scale - 0.5f, 0.f);
    Tap t;
    t.i0 = min((int)src, in - 1);
    t.i1 = min(t.i0 + 1, in - 1);
    t.w1 = src - (float)t.i0;
    t.w0 = 1.f - t.w1;
    return t;
}

template <typename T>
__global__ __launch_bounds__(256) void resize_kernel(const T* __restrict__ x, T* __restrict__ y, int B, int Hin, int Win, int Hout, int Wout,
                                                     int C, int ldx, int ldy) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)B * Hout * Wout * C) return;
    const int c = (int)(t % C);
    const int64_t pix = t / C;
    const int ox = (int)(pix % Wout);
    const int64_t q = pix / Wout;
    const int oy = (int)(q % Hout), b = (int)(q / Hout);
    const Tap ty = bilinear_tap(oy, Hin, Hout), tx = bilinear_tap(ox, Win, Wout);
    const T* xb = x + (int64_t)b * Hin * Win * ldx + c;
    const float v00 = Elem<T>::ld(xb + ((int64_t)ty.i0 * Win + tx.i0) * ldx), v01 = Elem<T>::ld(xb + ((int64_t)ty.i0 * Win + tx.i1) * ldx);
    const float v10 = Elem<T>::ld(xb + ((int64_t)ty.i1 * Win + tx.i0) * ldx), v11 = Elem<T>::ld(xb + ((int64_t)ty.i1 * Win + tx.i1) * ldx);
    Elem<T>::st(y + pix * ldy + c, ty.w0 * (tx.w0 * v00 + tx.w1 * v01) + ty.w1 * (tx.w0 * v10 + tx.w1 * v11));
}

template <typename T>
__global__ __launch_bounds__(256) void torgb_kernel(const T* __restrict__ rgb, float* __restrict__ acc, float* __restrict__ out, int B, int r, int T_,
                                                    int ld, int first) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)B * 3 * T_ * T_) return;
    const int ox = (int)(t % T_);
    int64_t q = t / T_;
    const int oy = (int)(q % T_); q /= T_;
    const int ch = (int)(q % 3), b = (int)(q / 3);
    const Tap ty = bilinear_tap(oy, r, T_), tx = bilinear_tap(ox, r, T_);
    const T* xb = rgb + (int64_t)b * r * r * ld + ch;
    const float v00 = Elem<T>::ld(xb + ((int64_t)ty.i0 * r + tx.i0) * ld), v01 = Elem<T>::ld(xb + ((int64_t)ty.i0 * r + tx.i1) * ld);
    const float v10 = Elem<T>::ld(xb + ((int64_t)ty.i1 * r + tx.i0) * ld), v11 = Elem<T>::ld(xb + ((int64_t)ty.i1 * r + tx.i1) * ld);
    const float up = ty.w0 * (tx.w0 * v00 + tx.w1 * v01) + ty.w1 * (tx.w0 * v10 + tx.w1 * v11);
    const float s = first ? up : acc[t] + up;
    acc[t] = s;
    if (out != nullptr) out[t] = tanhf(s);
}

// ---------------------------------------------------------------- standard normals (Box-Muller over the samplers' hash)
__device__ __forceinline__ float normal_from_bits(uint32_t h0, uint32_t h1) {
    const float u1 = (float)(2u * (h0 >> 9) + 1u) * 5.9604644775390625e-8f;         // odd multiple of 2^-24 in (0, 1): exact
    const float u2 = (float)(h1 >> 8) * 5.9604644775390625e-8f;                     // multiple of 2^-24 in [0, 1): exact
    return sqrtf(-2.0f * logf(u1)) * cospif(2.0f * u2);
}

__global__ __launch_bounds__(256) void normal_planes_kernel(float* __restrict__ out, uint32_t mix, int B, int P) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)B * P) return;
    const uint32_t b = (uint32_t)(t / P), p = (uint32_t)(t % P);
    out[t] = normal_from_bits(gumbel_bits(mix, b, 2u * p), gumbel_bits(mix, b, 2u * p + 1u));
}

__global__ __launch_bounds__(256) void normal_from_bits_kernel(const uint32_t* __restrict__ h0, const uint32_t* __restrict__ h1, float* __restrict__ z,
                                                               int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) z[i] = normal_from_bits(h0[i], h1[i]);
}

static inline unsigned blocks256(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace xl

using namespace xl;

extern "C" int xl_conv2d_nhwc(const void* x, const void* w, const float* bias, void* y, const void* aux, const float* mean, const float* rstd,
                              const float* noise, float noise_w, float slope, int B, int H, int W, int Cin, int Cout, int ks, int groups,
                              int ldx, int ldy, int ldaux, int epilogue, int dtype, void* stream) {
    XL_CHECK_ARG(x && w && y, XL_ERR_BAD_ARG, "xl_conv2d_nhwc: null x, w or y");
    XL_CHECK_ARG(dtype == XL_F32 || dtype == XL_BF16, XL_ERR_BAD_DTYPE, "xl_conv2d_nhwc: bad dtype %d", dtype);
    XL_CHECK_ARG(ks == 1 || ks == 3, XL_ERR_BAD_ARG, "xl_conv2d_nhwc: ks=%d (1 or 3)", ks);
    XL_CHECK_ARG(epilogue >= XL_CONV_NONE && epilogue <= XL_CONV_SPADE, XL_ERR_BAD_ARG, "xl_conv2d_nhwc: unknown epilogue %d", epilogue);
    XL_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 1, XL_ERR_BAD_SHAPE, "xl_conv2d_nhwc: B=%d H=%d W=%d Cin=%d Cout=%d", B, H, W,
                 Cin, Cout);
    XL_CHECK_ARG(groups >= 1 && Cin % groups == 0 && Cout % groups == 0, XL_ERR_BAD_SHAPE, "xl_conv2d_nhwc: groups=%d does not divide Cin=%d and Cout=%d",
                 groups, Cin, Cout);
    const bool spade = epilogue == XL_CONV_SPADE;
    XL_CHECK_ARG(!spade || (Cout % 2 == 0 && groups == 1 && aux && mean && rstd), XL_ERR_BAD_ARG,
                 "xl_conv2d_nhwc: XL_CONV_SPADE needs an even Cout (%d), groups == 1 (%d), aux, mean and rstd", Cout, groups);
    XL_CHECK_ARG(epilogue != XL_CONV_ADD || aux, XL_ERR_BAD_ARG, "xl_conv2d_nhwc: XL_CONV_ADD needs aux");
    const int Cy = spade ? Cout / 2 : Cout;
    const bool has_aux = spade || epilogue == XL_CONV_ADD;
    XL_CHECK_ARG(ldx >= Cin && ldy >= Cy && (!has_aux || ldaux >= Cy), XL_ERR_BAD_SHAPE,
                 "xl_conv2d_nhwc: pixel strides ldx=%d ldy=%d ldaux=%d below the channel counts %d / %d", ldx, ldy, ldaux, Cin, Cy);
    const int64_t npix = (int64_t)B * H * W;
    const int ldmax = ldx > ldy ? (ldx > ldaux ? ldx : ldaux) : (ldy > ldaux ? ldy : ldaux);
    XL_CHECK_ARG(npix * ldmax < (1ll << 31), XL_ERR_BAD_SHAPE, "xl_conv2d_nhwc: B*H*W*ld = %lld reaches 2^31", (long long)(npix * ldmax));
    ConvArgs a;
    a.x = x; a.w = w; a.bias = bias; a.y = y; a.aux = has_aux ? aux : nullptr; a.mean = mean; a.rstd = rstd; a.noise = spade ? noise : nullptr;
    a.noise_w = noise_w; a.slope = slope;
    a.B = B; a.H = H; a.W = W; a.Cin = Cin; a.Cout = Cout; a.ks = ks; a.groups = groups; a.ldx = ldx; a.ldy = ldy; a.ldaux = ldaux; a.epi = epilogue;
    a.tiles_x = (W + CT_W - 1) / CT_W; a.tiles_y = (H + CT_H - 1) / CT_H;
    hipStream_t st = (hipStream_t)stream;
    const int pad = ks >> 1;
    const int lds = (CT_H + 2 * pad) * (CT_W + 2 * pad) * (Cin * 2 + 16);
    const bool mfma = dtype == XL_BF16 && groups == 1 && Cin % 16 == 0 && (Cout == 32 || Cout == 64 || Cout == 128) && lds <= CONV_LDS_MAX &&
                      ldx % 8 == 0 && ldy % 4 == 0 && (!has_aux || ldaux % 4 == 0) && aligned16(x) && aligned16(w) && aligned16(y) &&
                      aligned16(a.aux) && aligned16(bias) && (!spade || (bias && aligned16(mean) && aligned16(rstd))) &&
                      (int64_t)B * a.tiles_y * a.tiles_x < (1ll << 31);
    if (mfma) {
        hipError_t e = Cout == 32 ? launch_conv_mfma<1>(a, lds, st) : Cout == 64 ? launch_conv_mfma<2>(a, lds, st) : launch_conv_mfma<4>(a, lds, st);
        if (e != hipSuccess) { set_error("xl_conv2d_nhwc: hipFuncSetAttribute: %s", hipGetErrorString(e)); return XL_ERR_HIP; }
    } else {
        const unsigned nb = blocks256(npix * Cy);
        if (dtype == XL_F32) hipLaunchKernelGGL(conv_generic_kernel<float>, dim3(nb), dim3(256), 0, st, a);
        else hipLaunchKernelGGL(conv_generic_kernel<bf16_t>, dim3(nb), dim3(256), 0, st, a);
    }
    XL_CHECK_LAUNCH();
    return XL_OK;
}

extern "C" int xl_instnorm_stats(const void* x, float* mean, float* rstd, float* ws, int64_t ws_floats, int B, int HW, int C, int ld, float eps,
                                 int dtype, void* stream) {
    XL_CHECK_ARG(x && mean && rstd && ws, XL_ERR_BAD_ARG, "xl_instnorm_stats: null argument");
    XL_CHECK_ARG(dtype == XL_F32 || dtype == XL_BF16, XL_ERR_BAD_DTYPE, "xl_instnorm_stats: bad dtype %d", dtype);
    XL_CHECK_ARG(B >= 1 && B <= 65535 && HW >= 1 && C >= 1 && ld >= C && (int64_t)B * HW * ld < (1ll << 31) && eps > 0.f, XL_ERR_BAD_SHAPE,
                 "xl_instnorm_stats: B=%d (1..65535) HW=%d C=%d ld=%d eps=%g", B, HW, C, ld, (double)eps);
    const int nchunks = (HW + XL_INSTNORM_CHUNK - 1) / XL_INSTNORM_CHUNK;
    XL_CHECK_ARG(ws_floats >= 2ll * B * nchunks * C, XL_ERR_BAD_ARG, "xl_instnorm_stats: workspace of %lld floats, %lld needed", (long long)ws_floats,
                 2ll * B * nchunks * C);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == XL_F32) hipLaunchKernelGGL(instnorm_stage1_kernel<float>, dim3(nchunks, B), dim3(256), 0, st, (const float*)x, ws, HW, C, ld, nchunks);
    else hipLaunchKernelGGL(instnorm_stage1_kernel<bf16_t>, dim3(nchunks, B), dim3(256), 0, st, (const bf16_t*)x, ws, HW, C, ld, nchunks);
    XL_CHECK_LAUNCH();
    hipLaunchKernelGGL(instnorm_stage2_kernel, dim3(blocks256((int64_t)B * C)), dim3(256), 0, st, ws, mean, rstd, B, HW, C, nchunks, eps);
    XL_CHECK_LAUNCH();
    return XL_OK;
}

extern "C" int xl_resize_bilinear_nhwc(const void* x, void* y, int B, int Hin, int Win, int Hout, int Wout, int C, int ldx, int ldy, int dtype,
                                       void* stream) {
    XL_CHECK_ARG(x && y, XL_ERR_BAD_ARG, "xl_resize_bilinear_nhwc: null argument");
    XL_CHECK_ARG(dtype == XL_F32 || dtype == XL_BF16, XL_ERR_BAD_DTYPE, "xl_resize_bilinear_nhwc: bad dtype %d", dtype);
    XL_CHECK_ARG(B >= 1 && Hin >= 1 && Win >= 1 && Hout >= 1 && Wout >= 1 && C >= 1 && ldx >= C && ldy >= C &&
                     (int64_t)B * Hin * Win * ldx < (1ll << 31) && (int64_t)B * Hout * Wout * ldy < (1ll << 31),
                 XL_ERR_BAD_SHAPE, "xl_resize_bilinear_nhwc: B=%d %dx%d -> %dx%d C=%d ldx=%d ldy=%d", B, Hin, Win, Hout, Wout, C, ldx, ldy);
    const unsigned nb = blocks256((int64_t)B * Hout * Wout * C);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == XL_F32) hipLaunchKernelGGL(resize_kernel<float>, dim3(nb), dim3(256), 0, st, (const float*)x, (float*)y, B, Hin, Win, Hout, Wout, C, ldx, ldy);
    else hipLaunchKernelGGL(resize_kernel<bf16_t>, dim3(nb), dim3(256), 0, st, (const bf16_t*)x, (bf16_t*)y, B, Hin, Win, Hout, Wout, C, ldx, ldy);
    XL_CHECK_LAUNCH();
    return XL_OK;
}

extern "C" int xl_torgb_accum(const void* rgb, float* acc, float* out, int B, int r, int T, int ld, int first, int dtype, void* stream) {
    XL_CHECK_ARG(rgb && acc, XL_ERR_BAD_ARG, "xl_torgb_accum: null argument");
    XL_CHECK_ARG(dtype == XL_F32 || dtype == XL_BF16, XL_ERR_BAD_DTYPE, "xl_torgb_accum: bad dtype %d", dtype);
    XL_CHECK_ARG(B >= 1 && r >= 1 && T >= 1 && ld >= 3 && (int64_t)B * r * r * ld < (1ll << 31) && (int64_t)B * 3 * T * T < (1ll << 31),
                 XL_ERR_BAD_SHAPE, "xl_torgb_accum: B=%d r=%d T=%d ld=%d", B, r, T, ld);
    const unsigned nb = blocks256((int64_t)B * 3 * T * T);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == XL_F32) hipLaunchKernelGGL(torgb_kernel<float>, dim3(nb), dim3(256), 0, st, (const float*)rgb, acc, out, B, r, T, ld, first);
    else hipLaunchKernelGGL(torgb_kernel<bf16_t>, dim3(nb), dim3(256), 0, st, (const bf16_t*)rgb, acc, out, B, r, T, ld, first);
    XL_CHECK_LAUNCH();
    return XL_OK;
}

extern "C" int xl_normal_planes(float* out, uint64_t seed, int site, int B, int P, void* stream) {
    XL_CHECK_ARG(out != nullptr && site >= 0, XL_ERR_BAD_ARG, "xl_normal_planes: null out or site %d < 0", site);
    XL_CHECK_ARG(B >= 1 && P >= 1 && P < (1 << 30) && (int64_t)B * P < (1ll << 31), XL_ERR_BAD_SHAPE, "xl_normal_planes: B=%d P=%d", B, P);
    const uint64_t s = seed + (uint64_t)site * 0x9E3779B97F4A7C15ull;
    hipLaunchKernelGGL(normal_planes_kernel, dim3(blocks256((int64_t)B * P)), dim3(256), 0, (hipStream_t)stream, out,
                       (uint32_t)s ^ (uint32_t)(s >> 32) * 0xC2B2AE3Du, B, P);          // = gumbel_seed_mix (csrc/common.h)
    XL_CHECK_LAUNCH();
    return XL_OK;
}

extern "C" int xl_normal_from_bits(const uint32_t* h0, const uint32_t* h1, float* z, int n, void* stream) {
    XL_CHECK_ARG(h0 && h1 && z && n > 0, XL_ERR_BAD_ARG, "xl_normal_from_bits: bad args");
    hipLaunchKernelGGL(normal_from_bits_kernel, dim3(blocks256(n)), dim3(256), 0, (hipStream_t)stream, h0, h1, z, n);
    XL_CHECK_LAUNCH();
    return XL_OK;
}
