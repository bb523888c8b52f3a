// The training step of the deformable block's dense front (gf_deform_logits_forward, deform_dense.hip): the op is linear, so
// its forward saves nothing and IS the inference launch; this file holds the backward and its size query.  The contract:
// include/gf_hip.h; the design and the measured numbers: DESIGN.md §3.13g.  A translation unit of its own: deform_dense.hip's
// kernels stay the instruction streams they are.
//
// Three kernels, no atomics, §3.13b's organisation.  (1) The data backward on the forward's tile and register layout: the
// gradient columns go through product_t in groups of up to 128 -- raw's in ascending order (against Ww), then the learned
// columns (one group, against Wl).  A group's product is one accumulator chain from zero, and the groups' results are added in
// that order: a single chain over all of raw's columns (432 steps at Nw = 864) misses the tests' bound, chains of 64 steps
// with a sum behind them hold it.  grad_embed = (G0 + G1) + .. is stored when raw's groups are done,
// grad_feature = grad_embed + L behind the learned group: one pass, one accumulator set, the same bits where L is absent.
// Per tile it also writes the sums over its rows of the gradient columns (the bias gradients' partials, in double).  (2) The
// weight gradients per block of kLogitsWgRows rows, a 128 x 128 piece per group of 128 gradient columns: dWw = g_r^T (f + e),
// the sum formed in registers, dWl = g_l^T f.  (3) One fixed-order sum of the partials into the caller's gradient tensors:
// stored, not accumulated.
#include "gf_deform.hpp"
#include "gf_rows_bwd.hpp"

namespace gf {

constexpr int kLogitsWgRows = GF_DEFORM_LOGITS_WGRAD_ROWS;
static_assert(kLogitsWgRows % kRowTile == 0, "a weight-gradient block is whole tiles");
constexpr int kLogitsLearnedPad = 32;     // the learned columns' slot in a partial: GF_DEFORM_MAX_LEARNED, one register block
static_assert(GF_DEFORM_MAX_LEARNED <= kLogitsLearnedPad, "the learned columns are one register block");
static_assert(4 * 32 * kLogitsLearnedPad <= 32 * kRowTPitch, "the four waves' runs of grad_learned fit one staging buffer");

constexpr int kLogitsGroup = 128;      // gradient columns a product: four register blocks
__device__ __forceinline__ void add_rows(f32x16 (&acc)[4], const f32x16 (&part)[4])
{
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[b] += part[b];
}

// tile_sum (gf_rows_bwd.hpp) in double, the tile's sum rounded once to float: the bias gradients are plain sums of the
// cotangent's columns, and where a column nearly cancels a float tree's rounding is what is left of it
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ double dpp_add_f64(double v)
{
    const uint64_t b = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)b, CTRL, ROW_MASK, 0xf, true);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(b >> 32), CTRL, ROW_MASK, 0xf, true);
    return v + __builtin_bit_cast(double, (uint64_t)hi << 32 | lo);
}
__device__ __forceinline__ double sum32_last_f64(double v)      // sum32_last's order; valid in lanes 31 and 63
{
    v = dpp_add_f64<0x111>(v);
    v = dpp_add_f64<0x112>(v);
    v = dpp_add_f64<0x114>(v);
    v = dpp_add_f64<0x118>(v);
    return dpp_add_f64<0x142, 0xa>(v);
}
template <int NB, class F>
__device__ __forceinline__ void tile_sum_f64(F f, bool valid, double (*s_part)[128], float *dst, int t, int wv, int j, int h)
{
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const double s = sum32_last_f64(valid ? (double)f(b, r) : 0.0);
            if (j == 31) s_part[wv][32 * b + 8 * (r >> 2) + 4 * h + (r & 3)] = s;
        }
    __syncthreads();
    if (t < 32 * NB) dst[t] = (float)((s_part[0][t] + s_part[1][t]) + (s_part[2][t] + s_part[3][t]));
    __syncthreads();
}

struct DeformLogitsBwdArgs {
    const float *gl, *gr;      // the cotangents (null: zero)
    const float *wl, *ww;
    float *gf, *ge;            // grad_feature, grad_embed (null: not asked for)
    float *vpart;              // [tiles][vlen]: a tile's sums of | the learned columns (32, with K3 > 0) | raw's (128 per group) |
    int n, K3, Nw, vlen, want_bl, want_bw;
};

__global__ __launch_bounds__(256) void gf_deform_logits_bwd_kernel(DeformLogitsBwdArgs a)
{
    __shared__ float s_t[2][32 * kRowTPitch];
    __shared__ double s_part[4][128];
    const int t = threadIdx.x, l = t & 63, wv = t >> 6, j = l & 31, h = l >> 5;
    const int row0 = blockIdx.x * kRowTile + wv * 32;
    const bool valid = row0 + j < a.n;      // a row past n walks with a zero gradient and stores nothing
    const size_t row = (size_t)min(row0 + j, a.n - 1);
    const bool chain = a.gf || a.ge;
    float *vp = a.vpart + (size_t)blockIdx.x * a.vlen;

    f32x16 acc[4];
    zero_rows(acc);
    if (a.gr && (chain || a.want_bw)) {
        const int groups = (a.Nw + kLogitsGroup - 1) / kLogitsGroup;
        float *vraw = vp + (a.K3 > 0 ? kLogitsLearnedPad : 0);
#pragma unroll 1
        for (int q = 0; q < groups; ++q) {
            const int col0 = kLogitsGroup * q, ncols = min(kLogitsGroup, a.Nw - col0);
            auto group = [&](auto nc) {
                constexpr int NC = decltype(nc)::value;
                f32x16 g[NC];
#pragma unroll
                for (int b = 0; b < NC; ++b)
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        const int col = col0 + 32 * b + 8 * m + 4 * h;      // (Nw is a multiple of 4: a float4 is whole or absent)
                        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (valid && col < a.Nw) v = ld4(a.gr + row * a.Nw + col);
                        g[b][4 * m] = v.x; g[b][4 * m + 1] = v.y; g[b][4 * m + 2] = v.z; g[b][4 * m + 3] = v.w;
                    }
                if (a.want_bw) tile_sum_f64<NC>([&](int b, int r) { return g[b][r]; }, valid, s_part, vraw + col0, t, wv, j, h);
                if (chain) {
                    f32x16 part[4];
                    zero_rows(part);
                    product_t<NC, true>(part, g, a.ww + (size_t)col0 * kDeformE, kDeformE, ncols, s_t[0], s_t[1], t, j, h);
                    add_rows(acc, part);
                }
            };
            switch ((ncols + 31) / 32) {
            case 1: group(std::integral_constant<int, 1>()); break;
            case 2: group(std::integral_constant<int, 2>()); break;
            case 3: group(std::integral_constant<int, 3>()); break;
            default: group(std::integral_constant<int, 4>()); break;
            }
        }
    }
    if (valid && a.ge) store_row_regs(a.ge + row * kDeformE, acc, h);      // (G0 + G1) + ..

    if (a.gl && (a.gf || a.want_bl)) {
        // a row of grad_learned is K3 floats, not 16-byte aligned: the wave's rows are one run of memory, taken through LDS
        // (s_t[1]: every wave is behind the last product's closing barrier, and a product of one chunk writes s_t[0] only)
        float *so = s_t[1] + wv * (32 * kLogitsLearnedPad);
        const int count = min(32, a.n - row0) * a.K3;
        for (int k = l; k < count; k += 64) so[k] = a.gl[(size_t)row0 * a.K3 + k];
        __syncthreads();
        f32x16 g[1];
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int col = 8 * m + 4 * h + i;
                float v = 0.f;
                if (valid && col < a.K3) v = so[j * a.K3 + col];
                g[0][4 * m + i] = v;
            }
        if (a.want_bl) tile_sum_f64<1>([&](int, int r) { return g[0][r]; }, valid, s_part, vp, t, wv, j, h);
        if (a.gf) {
            f32x16 part[4];
            zero_rows(part);
            product_t<1, true>(part, g, a.wl, kDeformE, a.K3, s_t[0], s_t[1], t, j, h);
            add_rows(acc, part);
        }
    }
    if (valid && a.gf) store_row_regs(a.gf + row * kDeformE, acc, h);      // ((G0 + G1) + ..) + L
}

struct DeformLogitsWgArgs {
    const float *gl, *gr, *f, *e;
    float *wpart;          // [blocks][wlen]: | dWw's rows [Nw][128] | dWl's [32][128] (with K3 > 0) |
    size_t wlen;
    int n, K3, Nw, piece0;     // blockIdx.y + piece0: raw's group of 128 columns, or (== groups) the learned columns
};

// A row block's piece of g^T x, A = g[row][o] and B = x[row][k], two rows a step; a wave owns 32 rows o (wgrad_rows).  A lane
// whose column o lies past the width walks the last column instead and stores nothing; a wave without a column returns
__global__ __launch_bounds__(256) void gf_deform_logits_wgrad_kernel(DeformLogitsWgArgs a)
{
    const int blk = blockIdx.x, piece = blockIdx.y + a.piece0;
    const int t = threadIdx.x, l = t & 63, wv = t >> 6, j = l & 31, h = l >> 5;
    const int r0 = blk * kLogitsWgRows, r1 = min(a.n, r0 + kLogitsWgRows);
    const bool raw = piece < (a.Nw + 127) / 128;
    const int col0 = raw ? 128 * piece : 0, width = raw ? a.Nw : a.K3;
    if (col0 + 32 * wv >= width) return;
    const float *left = (raw ? a.gr : a.gl) + min(col0 + 32 * wv + j, width - 1);
    const float gv[4] = {1.f, 1.f, 1.f, 1.f}, ev[4] = {0.f, 0.f, 0.f, 0.f};
    f32x16 acc[4];
    zero_rows(acc);
    if (raw && a.e) wgrad_rows<kWgSum>(acc, left, (size_t)width, 0, a.f + j, a.e + j, kDeformE, 0, nullptr, gv, ev, r0, r1, r1, h);
    else wgrad_rows<kWgAsIs>(acc, left, (size_t)width, 0, a.f + j, nullptr, kDeformE, 0, nullptr, gv, ev, r0, r1, r1, h);
    float *dst = a.wpart + (size_t)blk * a.wlen + (size_t)(raw ? col0 : a.Nw) * kDeformE + j;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = 32 * wv + 8 * (r >> 2) + 4 * h + (r & 3);
            if (col0 + o < width) dst[(size_t)o * kDeformE + 32 * cb] = acc[cb][r];
        }
}

static const char *const kDeformLogitsName[GF_DEFORM_LOGITS_PARAMS] = {"kps_generator.learnable_fc.weight", "kps_generator.learnable_fc.bias",
                                                                        "weights_fc.weight", "weights_fc.bias"};

// what gf_deform_logits_forward checks of the sizes and the parameter table, under the name `fn` of the one called
static int deform_logits_check_sizes(const char *fn, int n, int E, int K3, int Nw)
{
    GF_REFUSE_AS(fn, E == kDeformE, "E = %d: only embed_dims = 128 is supported", E);
    GF_REFUSE_AS(fn, K3 >= 0 && K3 <= GF_DEFORM_MAX_LEARNED, "K3 = %d: the learned columns 3 K must be 0 .. %d", K3, GF_DEFORM_MAX_LEARNED);
    GF_REFUSE_AS(fn, Nw >= 4 && Nw % 4 == 0, "Nw = %d: the logits' width must be a positive multiple of 4", Nw);
    GF_REFUSE_AS(fn, n >= 0, "n = %d is negative", n);
    return GF_OK;
}
static int deform_logits_check_params(const char *fn, int K3, const void *const *params)
{
    GF_REFUSE_AS(fn, params, "null params");
    const float *const *p = reinterpret_cast<const float *const *>(params);
    for (int i = K3 > 0 ? 0 : 2; i < GF_DEFORM_LOGITS_PARAMS; ++i) {
        GF_REFUSE_AS(fn, p[i], "%s is missing", kDeformLogitsName[i]);
        GF_REFUSE_AS(fn, !misaligned16(p[i]), "%s is not 16-byte aligned", kDeformLogitsName[i]);
    }
    return GF_OK;
}
static bool misaligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; }

// The workspace, sized and carved by one function (a null base: sizes only).
struct DeformLogitsWork { float *vpart, *wpart; int tiles, blocks, groups, vlen; size_t wlen, bytes; };
static DeformLogitsWork deform_logits_carve_work(void *base, int n, int K3, int Nw)
{
    Carver c(base);
    DeformLogitsWork w;
    const int pad = K3 > 0 ? kLogitsLearnedPad : 0;
    w.tiles = (n + kRowTile - 1) / kRowTile;
    w.blocks = (n + kLogitsWgRows - 1) / kLogitsWgRows;
    w.groups = (Nw + 127) / 128;
    w.vlen = pad + 128 * w.groups;
    w.wlen = (size_t)(Nw + pad) * kDeformE;
    w.vpart = c.take<float>((size_t)w.tiles * w.vlen);
    w.wpart = c.take<float>((size_t)w.blocks * w.wlen);
    w.bytes = c.bytes();
    return w;
}

}  // namespace gf

extern "C" int gf_deform_logits_train_sizes(int n, int E, int K3, int Nw, size_t *saved_bytes, size_t *workspace_bytes)
{
    using namespace gf;
    const char *fn = __func__;
    if (int rc = deform_logits_check_sizes(fn, n, E, K3, Nw)) return rc;
    GF_REFUSE_AS(fn, saved_bytes && workspace_bytes, "null pointer");
    *saved_bytes = 0;     // the op is linear
    *workspace_bytes = deform_logits_carve_work(nullptr, n, K3, Nw).bytes;
    return GF_OK;
}

extern "C" int gf_deform_logits_backward(int n, int E, int K3, int Nw, const float *feature, const float *embed, const void *const *params,
                                         const float *grad_learned, const float *grad_raw, float *grad_feature, float *grad_embed,
                                         void *const *grad_params, void *workspace, size_t workspace_bytes, void *stream_)
{
    using namespace gf;
    const char *fn = __func__;
    if (int rc = deform_logits_check_sizes(fn, n, E, K3, Nw)) return rc;
    if (int rc = deform_logits_check_params(fn, K3, params)) return rc;
    const float *const *p = reinterpret_cast<const float *const *>(params);
    GF_REFUSE_AS(fn, !(grad_learned && K3 == 0), "grad_learned with K3 = %d: there are no learned columns", K3);
    GF_REFUSE_AS(fn, grad_params, "null grad_params");
    float *const *gp = reinterpret_cast<float *const *>(grad_params);
    bool any = false;
    for (int i = 0; i < GF_DEFORM_LOGITS_PARAMS; ++i) {
        GF_REFUSE_AS(fn, !gp[i] || (p[i] && (i >= 2 || K3 > 0)), "a gradient for %s, which is absent", kDeformLogitsName[i]);
        GF_REFUSE_AS(fn, i < 2 ? !misaligned4(gp[i]) : !misaligned16(gp[i]), "the gradient of %s is not %d-byte aligned", kDeformLogitsName[i], i < 2 ? 4 : 16);
        any = any || gp[i];
    }
    GF_REFUSE_AS(fn, !misaligned16(feature), "instance_feature is not 16-byte aligned");
    GF_REFUSE_AS(fn, !misaligned16(embed), "anchor_embed is not 16-byte aligned");
    GF_REFUSE_AS(fn, !misaligned4(grad_learned), "grad_learned is not 4-byte aligned");
    GF_REFUSE_AS(fn, !misaligned16(grad_raw), "grad_raw is not 16-byte aligned");
    GF_REFUSE_AS(fn, !misaligned16(grad_feature), "grad_feature is not 16-byte aligned");
    GF_REFUSE_AS(fn, !misaligned16(grad_embed), "grad_embed is not 16-byte aligned");
    GF_REFUSE_AS(fn, !misaligned16(workspace), "workspace is not 16-byte aligned");
    const bool need_work = n > 0 && any;
    const DeformLogitsWork ws = deform_logits_carve_work(need_work ? workspace : nullptr, n, K3, Nw);
    if (n > 0) GF_REFUSE_AS(fn, feature, "null pointer: instance_feature");
    if (need_work) {
        GF_REFUSE_AS(fn, workspace, "workspace is null");
        GF_CHECK_WORKSPACE_AS(fn, "workspace", workspace_bytes, ws.bytes);
    }
    // every output against every input, the workspace and the outputs before it
    const size_t in_bytes = (size_t)n * kDeformE * 4;
    const size_t pbytes[GF_DEFORM_LOGITS_PARAMS] = {(size_t)K3 * kDeformE * 4, (size_t)K3 * 4, (size_t)Nw * kDeformE * 4, (size_t)Nw * 4};
    struct Range { const void *p; size_t bytes; const char *what; };
    const Range ins[] = {{feature, in_bytes, "an input"}, {embed, in_bytes, "an input"}, {grad_learned, (size_t)n * K3 * 4, "an input"},
                         {grad_raw, (size_t)n * Nw * 4, "an input"}, {K3 > 0 ? p[0] : nullptr, pbytes[0], "an input"},
                         {K3 > 0 ? p[1] : nullptr, pbytes[1], "an input"}, {p[2], pbytes[2], "an input"}, {p[3], pbytes[3], "an input"},
                         {workspace, need_work ? ws.bytes : 0, "the workspace"}};
    const Range outs[] = {{grad_feature, in_bytes, "grad_feature"}, {grad_embed, in_bytes, "grad_embed"},
                          {gp[0], pbytes[0], "the gradient of kps_generator.learnable_fc.weight"},
                          {gp[1], pbytes[1], "the gradient of kps_generator.learnable_fc.bias"},
                          {gp[2], pbytes[2], "the gradient of weights_fc.weight"}, {gp[3], pbytes[3], "the gradient of weights_fc.bias"}};
    for (size_t o = 0; o < sizeof(outs) / sizeof(outs[0]); ++o) {
        for (const Range &in : ins) GF_REFUSE_AS(fn, !overlap(outs[o].p, outs[o].bytes, in.p, in.bytes), "%s aliases %s", outs[o].what, in.what);
        for (size_t q = 0; q < o; ++q)
            GF_REFUSE_AS(fn, !overlap(outs[o].p, outs[o].bytes, outs[q].p, outs[q].bytes), "%s aliases %s", outs[o].what, outs[q].what);
    }
    hipStream_t stream = (hipStream_t)stream_;
    const bool live_l = grad_learned != nullptr, live_r = grad_raw != nullptr;     // a null cotangent is zero
    if (n > 0) {
        const int want_bl = gp[1] && live_l, want_bw = gp[3] && live_r;
        if (grad_feature || grad_embed || want_bl || want_bw) {
            DeformLogitsBwdArgs b{grad_learned, grad_raw, p[0], p[2], grad_feature, grad_embed, ws.vpart, n, K3, Nw, ws.vlen, want_bl, want_bw};
            hipLaunchKernelGGL(gf_deform_logits_bwd_kernel, dim3(ws.tiles), dim3(256), 0, stream, b);
            GF_CHECK_LAUNCH();
        }
        const bool wg_r = gp[2] && live_r, wg_l = gp[0] && live_l;
        if (wg_r || wg_l) {
            DeformLogitsWgArgs g{grad_learned, grad_raw, feature, embed, ws.wpart, ws.wlen, n, K3, Nw, wg_r ? 0 : ws.groups};
            hipLaunchKernelGGL(gf_deform_logits_wgrad_kernel, dim3(ws.blocks, (wg_r ? ws.groups : 0) + (wg_l ? 1 : 0)), dim3(256), 0, stream, g);
            GF_CHECK_LAUNCH();
        }
    }
    // the sums, in the table's order; a zero cotangent or n == 0: no partials, zeros are stored
    RowsSumArgs<GF_DEFORM_LOGITS_PARAMS> sa{};     // sums in double, a thread per element
    int nj = 0, longest = 0;
    auto job = [&](int i, const float *base, size_t at, size_t stride, int count, int len, bool live) {
        if (!gp[i]) return;
        const bool has = n > 0 && live;
        sa.job[nj++] = RowsSumJob{has ? base + at : nullptr, gp[i], stride, has ? count : 0, len, 0, 1};
        longest = len > longest ? len : longest;
    };
    const int pad = K3 > 0 ? kLogitsLearnedPad : 0;
    job(0, ws.wpart, (size_t)Nw * kDeformE, ws.wlen, ws.blocks, K3 * kDeformE, live_l);
    job(1, ws.vpart, 0, (size_t)ws.vlen, ws.tiles, K3, live_l);
    job(2, ws.wpart, 0, ws.wlen, ws.blocks, Nw * kDeformE, live_r);
    job(3, ws.vpart, (size_t)pad, (size_t)ws.vlen, ws.tiles, Nw, live_r);
    if (nj > 0) {
        hipLaunchKernelGGL((rows_sum_kernel<double, GF_DEFORM_LOGITS_PARAMS>), dim3((longest + 255) / 256, nj), dim3(256), 0, stream, sa);
        GF_CHECK_LAUNCH();
    }
    return GF_OK;
}
