// Caption-image matching (include/xlxmert_hip.h, section "caption-image matching"): xl_pair_expand fills the first cross layer's
// input for a chunk of (caption, image) pairs from the outputs of ONE language stack over the captions and ONE visual stack over the
// images; xl_match_rank turns the relationship logits of the chunks into margins, probabilities, top-k lists and target ranks.
// Both move or compare values only (one subtraction, one exp, one add and one divide per pair aside): nothing here is a hot loop of
// arithmetic, the work is addressing -- rows move as 16-byte vectors, the ranking is one wave per query.
#include "common.h"

namespace xl {

constexpr int MATCH_MAX = 4096;          // captions / images of one xl_match_rank call
constexpr int MATCH_MAX_K = 32;

// first packed language row of pair p = n*M + m in the caption-major list of ALL pairs: the captions before n own M*lang_off[n] rows,
// the m pairs of caption n before this one m*len_n more.  64-bit: M * lang_off reaches 2^33 at the limits of the interface.
struct PairRows { int n, m, len; int64_t first; };
__device__ __forceinline__ PairRows pair_rows(const int* __restrict__ lang_off, const int* __restrict__ lang_len, int p, int M, int L) {
    PairRows r;
    r.n = p / M;
    r.m = p - r.n * M;
    const int o = lang_off[r.n];
    r.len = min(max(lang_len != nullptr ? lang_len[r.n] : lang_off[r.n + 1] - o, 0), L);      // (the host cannot check the offsets without a round trip: clamped to the capacity)
    r.first = (int64_t)M * o + (int64_t)r.m * r.len;
    return r;
}

struct ExpandArgs {
    const uint4* vis[2];        // visual stack output [M*V, d], up to two copies of the stream (fp32 value / bf16 rounding)
    const uint4* lang[2];       // language stack output, packed [lang_src_rows, d]
    uint4* dst[2];              // chunk X[0]: visual rows [B_c*V, d] then the language rows
    int vpr[2];                 // 16-byte vectors per row of each copy (0: copy absent)
    const int* lang_off;        // [N+1]
    const int* lang_len;        // [N] or NULL (dense chunk layout only): lengths of a source whose offsets are not their prefix sums
    int* loff_out;              // [B_c+1] (packed)
    int* lrows_out;             // [lang_rows_pad] (packed)
    uint8_t* kmask_out;         // [B_c, L]
    int M, V, L, pair_start, pair_count, B_c, packed, lang_src_rows, lang_rows_pad;
};

// One thread per 16-byte vector of one row task.  Row tasks, in this order:
//   [0, B_c*V)                    visual row (slot j, v)        <- image m's row v
//   [B_c*V, B_c*(V+L))            language position (slot j, l) <- caption n's row l, or (dense layout, l >= len_n) a zero row
//   [B_c*(V+L), +tail_rows)       packed layout: the zero rows that pad the packed rows to the row tile
// Slot j holds pair pair_start + min(j, pair_count-1): the slots of a ragged last chunk repeat its last real pair.
__global__ __launch_bounds__(256) void pair_expand_kernel(ExpandArgs a, int c, int tail_rows) {
    const int vpr = a.vpr[c];
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row_task = t / vpr;
    const int vec = (int)(t - row_task * vpr);
    const int n_vis = a.B_c * a.V, n_lang = a.B_c * a.L;
    if (row_task >= (int64_t)n_vis + n_lang + tail_rows) return;
    uint4* __restrict__ dst = a.dst[c];
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    if (row_task < n_vis) {
        const int j = (int)row_task / a.V, v = (int)row_task - j * a.V;
        const int p = a.pair_start + min(j, a.pair_count - 1);
        const int m = p % a.M;
        dst[row_task * vpr + vec] = a.vis[c][((int64_t)m * a.V + v) * vpr + vec];
        return;
    }
    uint4* __restrict__ ldst = dst + (int64_t)n_vis * vpr;
    const int last = a.pair_count - 1;
    const PairRows base = pair_rows(a.lang_off, a.lang_len, a.pair_start, a.M, a.L);
    if (row_task >= (int64_t)n_vis + n_lang) {          // pad tail of the packed rows (and of the row list)
        const PairRows pl = pair_rows(a.lang_off, a.lang_len, a.pair_start + last, a.M, a.L);
        const int64_t total = pl.first + (int64_t)pl.len * (a.B_c - last) - base.first;
        const int64_t r = total + (row_task - n_vis - n_lang);
        if (r < a.lang_rows_pad) {
            ldst[r * vpr + vec] = zero;
            if (vec == 0 && c == 0) a.lrows_out[r] = -1;
        }
        return;
    }
    const int q = (int)(row_task - n_vis);
    const int j = q / a.L, l = q - j * a.L;
    const int jr = min(j, last);
    const PairRows pr = pair_rows(a.lang_off, a.lang_len, a.pair_start + jr, a.M, a.L);
    const bool real = l < pr.len;
    const int64_t src_row = (int64_t)a.lang_off[pr.n] + l;
    const bool readable = real && src_row >= 0 && src_row < a.lang_src_rows;
    if (a.packed) {
        const int64_t off = pr.first + (int64_t)pr.len * (j - jr) - base.first;      // first chunk row of slot j
        const int64_t r = off + l;
        if (vec == 0 && c == 0) {
            a.kmask_out[q] = real ? 1 : 0;
            if (l == 0) {
                a.loff_out[j] = (int)off;
                if (j == a.B_c - 1) a.loff_out[a.B_c] = (int)(off + pr.len);
            }
            if (real && r < a.lang_rows_pad) a.lrows_out[r] = q;
        }
        if (real && r < a.lang_rows_pad) ldst[r * vpr + vec] = readable ? a.lang[c][src_row * vpr + vec] : zero;
    } else {
        if (vec == 0 && c == 0) a.kmask_out[q] = real ? 1 : 0;
        ldst[(int64_t)q * vpr + vec] = readable ? a.lang[c][src_row * vpr + vec] : zero;
    }
}

// ---------------------------------------------------------------- scores
__global__ __launch_bounds__(256) void match_scatter_kernel(const float* __restrict__ rel, float* __restrict__ margin,
                                                            float* __restrict__ prob, int pair_start, int pair_count) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= pair_count) return;
    const float2 x = *reinterpret_cast<const float2*>(rel + (int64_t)i * 8);
    const float mg = x.y - x.x;
    margin[pair_start + i] = mg;
    if (prob != nullptr) prob[pair_start + i] = 1.0f / (1.0f + expf(-mg));
}

// (value, index) of the order "margin descending, ties to the lower index"; a NaN margin ranks as -inf
__device__ __forceinline__ bool ranks_before(float va, int ia, float vb, int ib) { return va > vb || (va == vb && ia < ib); }
__device__ __forceinline__ float rank_key(float v) { return v != v ? -INFINITY : v; }

// One wave per query: query q of direction `dir` (0: caption q over the M images, candidate c = margin[q*M + c]; 1: image q over the
// N captions, candidate c = margin[c*M + q]).  top-k by k rounds of "the best candidate that ranks after the previous pick" -- every
// round a strided scan and one butterfly of comparisons, no arithmetic on the values: exact.  rank = the number of candidates that
// rank before the target.
__global__ __launch_bounds__(256) void match_rank_kernel(const float* __restrict__ margin, int N, int M, int k, int* __restrict__ topk_images,
                                                         int* __restrict__ topk_captions, const int* __restrict__ image_of_caption,
                                                         const int* __restrict__ caption_of_image, int* __restrict__ rank_t2i,
                                                         int* __restrict__ rank_i2t) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= N + M) return;
    const int dir = w >= N;
    const int q = dir ? w - N : w;
    const int n_cand = dir ? N : M;
    const float* base = dir ? margin + q : margin + (int64_t)q * M;
    const int64_t stride = dir ? M : 1;
    int* topk = dir ? topk_captions : topk_images;
    const int* target = dir ? caption_of_image : image_of_caption;
    int* rank = dir ? rank_i2t : rank_t2i;
    if (topk != nullptr) {
        float pv = INFINITY;
        int pi = -1;                    // the previous pick: nothing ranks before (+inf, -1)
        for (int r = 0; r < k; ++r) {
            float bv = -INFINITY;
            int bi = 0x7fffffff;        // "none": every candidate ranks before (-inf, INT_MAX)
            for (int c = lane; c < n_cand; c += 64) {
                const float v = rank_key(base[c * stride]);
                if (ranks_before(pv, pi, v, c) && ranks_before(v, c, bv, bi)) { bv = v; bi = c; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (ranks_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
            }
            if (lane == 0) topk[(int64_t)q * k + r] = bi;
            pv = bv;
            pi = bi;
        }
    }
    if (rank != nullptr && target != nullptr) {
        const int t = target[q];
        int cnt = 0;
        if (t >= 0 && t < n_cand) {
            const float tv = rank_key(base[t * stride]);
            for (int c = lane; c < n_cand; c += 64) cnt += ranks_before(rank_key(base[c * stride]), c, tv, t) ? 1 : 0;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
        } else {
            cnt = -1;
        }
        if (lane == 0) rank[q] = cnt;
    }
}

}  // namespace xl

using namespace xl;

extern "C" int xl_pair_expand(const void* vis, const void* lang, const void* vis2, const void* lang2, const int* lang_off, const int* lang_len,
                              void* x0, void* x0_2, int* chunk_off, int* chunk_rows, void* chunk_kmask, int N, int M, int V, int L, int d,
                              int pair_start, int pair_count, int B_c, int packed, int lang_src_rows, int lang_rows, int lang_rows_pad,
                              int dtype, int dtype2, void* stream) {
    XL_CHECK_ARG(vis && lang && lang_off && x0 && chunk_kmask, XL_ERR_BAD_ARG, "xl_pair_expand: null argument");
    XL_CHECK_ARG(!packed || (chunk_off && chunk_rows), XL_ERR_BAD_ARG, "xl_pair_expand: the packed layout needs chunk_off and chunk_rows");
    XL_CHECK_ARG(!packed || lang_len == nullptr, XL_ERR_BAD_ARG, "xl_pair_expand: lang_len goes with the dense chunk layout only");
    XL_CHECK_ARG((vis2 != nullptr) == (lang2 != nullptr) && (vis2 != nullptr) == (x0_2 != nullptr), XL_ERR_BAD_ARG,
                 "xl_pair_expand: the second copy of the stream needs vis2, lang2 and x0_2 together");
    XL_CHECK_ARG(dtype == XL_F32 || dtype == XL_BF16, XL_ERR_BAD_DTYPE, "xl_pair_expand: bad dtype %d", dtype);
    XL_CHECK_ARG(vis2 == nullptr || dtype2 == XL_F32 || dtype2 == XL_BF16, XL_ERR_BAD_DTYPE, "xl_pair_expand: bad dtype2 %d", dtype2);
    XL_CHECK_ARG(N >= 1 && M >= 1 && N <= MATCH_MAX && M <= MATCH_MAX && V >= 1 && L >= 1 && L <= 512 && d >= 8, XL_ERR_BAD_SHAPE,
                 "xl_pair_expand: N=%d M=%d (1..%d) V=%d L=%d (1..512) d=%d", N, M, MATCH_MAX, V, L, d);
    XL_CHECK_ARG(d % 8 == 0, XL_ERR_BAD_SHAPE, "xl_pair_expand: d=%d is not a multiple of 8 (rows move as 16-byte vectors)", d);
    XL_CHECK_ARG(B_c >= 1 && pair_count >= 1 && pair_count <= B_c && pair_start >= 0 && (int64_t)pair_start + pair_count <= (int64_t)N * M,
                 XL_ERR_BAD_ARG, "xl_pair_expand: pairs [%d, %d+%d) of %d x %d in a chunk of %d", pair_start, pair_start, pair_count, N, M, B_c);
    XL_CHECK_ARG((int64_t)B_c * (V + L) < (1ll << 30) && lang_src_rows >= 1, XL_ERR_BAD_SHAPE, "xl_pair_expand: B_c=%d V=%d L=%d lang_src_rows=%d",
                 B_c, V, L, lang_src_rows);
    XL_CHECK_ARG(packed ? (lang_rows >= 1 && lang_rows <= lang_rows_pad && (int64_t)lang_rows_pad <= (int64_t)B_c * L + 255)
                        : (lang_rows == B_c * L && lang_rows_pad == lang_rows),
                 XL_ERR_BAD_ARG, "xl_pair_expand: lang_rows=%d lang_rows_pad=%d for B_c*L=%d (%s)", lang_rows, lang_rows_pad, B_c * L,
                 packed ? "packed" : "dense");
    XL_CHECK_ARG(aligned16(vis) && aligned16(lang) && aligned16(x0) && aligned16(vis2) && aligned16(lang2) && aligned16(x0_2), XL_ERR_UNALIGNED,
                 "xl_pair_expand: buffers must be 16-byte aligned");
    ExpandArgs a;
    a.vis[0] = (const uint4*)vis; a.lang[0] = (const uint4*)lang; a.dst[0] = (uint4*)x0;
    a.vis[1] = (const uint4*)vis2; a.lang[1] = (const uint4*)lang2; a.dst[1] = (uint4*)x0_2;
    a.vpr[0] = d * (dtype == XL_F32 ? 4 : 2) / 16;
    a.vpr[1] = vis2 ? d * (dtype2 == XL_F32 ? 4 : 2) / 16 : 0;
    a.lang_off = lang_off; a.lang_len = lang_len; a.loff_out = chunk_off; a.lrows_out = chunk_rows; a.kmask_out = (uint8_t*)chunk_kmask;
    a.M = M; a.V = V; a.L = L; a.pair_start = pair_start; a.pair_count = pair_count; a.B_c = B_c; a.packed = packed ? 1 : 0;
    a.lang_src_rows = lang_src_rows; a.lang_rows_pad = lang_rows_pad;
    const int tail_rows = packed ? lang_rows_pad - lang_rows : 0;
    for (int c = 0; c < 2; ++c) {
        if (a.vpr[c] == 0) continue;
        const int64_t threads = ((int64_t)B_c * (V + L) + tail_rows) * a.vpr[c];
        hipLaunchKernelGGL(pair_expand_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, c, tail_rows);
        XL_CHECK_LAUNCH();
    }
    return XL_OK;
}

extern "C" int xl_match_rank(const float* rel, int pair_start, int pair_count, float* margin, float* prob, int N, int M, int rank_stage,
                             int k, int* topk_images, int* topk_captions, const int* image_of_caption, const int* caption_of_image,
                             int* rank_t2i, int* rank_i2t, void* stream) {
    XL_CHECK_ARG(margin != nullptr, XL_ERR_BAD_ARG, "xl_match_rank: null margin");
    XL_CHECK_ARG(N >= 1 && M >= 1 && N <= MATCH_MAX && M <= MATCH_MAX, XL_ERR_BAD_SHAPE, "xl_match_rank: N=%d M=%d (1..%d)", N, M, MATCH_MAX);
    XL_CHECK_ARG(rel != nullptr || rank_stage, XL_ERR_BAD_ARG, "xl_match_rank: nothing to do (no rel, no rank stage)");
    if (rel != nullptr)
        XL_CHECK_ARG(pair_count >= 1 && pair_start >= 0 && (int64_t)pair_start + pair_count <= (int64_t)N * M && aligned16(rel), XL_ERR_BAD_ARG,
                     "xl_match_rank: pairs [%d, %d+%d) of %d x %d", pair_start, pair_start, pair_count, N, M);
    if (rank_stage) {
        XL_CHECK_ARG((image_of_caption != nullptr) == (rank_t2i != nullptr) && (caption_of_image != nullptr) == (rank_i2t != nullptr),
                     XL_ERR_BAD_ARG, "xl_match_rank: a target array and its rank output come together");
        XL_CHECK_ARG(topk_images || topk_captions || rank_t2i || rank_i2t, XL_ERR_BAD_ARG, "xl_match_rank: rank stage without an output");
        if (topk_images || topk_captions)
            XL_CHECK_ARG(k >= 1 && k <= MATCH_MAX_K && (!topk_images || k <= M) && (!topk_captions || k <= N), XL_ERR_BAD_ARG,
                         "xl_match_rank: k=%d not in 1..min(%d, candidates) (N=%d M=%d)", k, MATCH_MAX_K, N, M);
    }
    if (rel != nullptr) {
        hipLaunchKernelGGL(match_scatter_kernel, dim3((pair_count + 255) / 256), dim3(256), 0, (hipStream_t)stream, rel, margin, prob,
                           pair_start, pair_count);
        XL_CHECK_LAUNCH();
    }
    if (rank_stage) {
        hipLaunchKernelGGL(match_rank_kernel, dim3((N + M + 3) / 4), dim3(256), 0, (hipStream_t)stream, margin, N, M, k, topk_images,
                           topk_captions, image_of_caption, caption_of_image, rank_t2i, rank_i2t);
        XL_CHECK_LAUNCH();
    }
    return XL_OK;
}
