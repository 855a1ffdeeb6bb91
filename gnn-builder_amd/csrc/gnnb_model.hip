// gnnb_model.hip -- the model handle of libgnnb_hip.so: validation of a description, and gnnb_model_create's weight upload --
// the canonical tensors plus the derived forms the kernels read (one helper each below), packed into ONE device blob.
// Reference: load_parameters once (gnnbuilder/templates/model.cpp.jinja:724-730).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "gnnb_host.h"

using namespace gnnb;

static int validate_desc(const gnnb_model_desc *d)
{
    if (!d)
        return fail(GNNB_ERR_INVALID, "null model description");
    if (conv_slots(d->conv_type) < 0)
        return fail(GNNB_ERR_INVALID, "unsupported conv_type %d", d->conv_type);
    if (d->num_layers < 0 || d->num_layers > GNNB_MAX_LAYERS)
        return fail(GNNB_ERR_INVALID, "num_layers %d out of range", d->num_layers);
    if (d->in_dim < 1 || d->out_dim < 1 || (d->num_layers > 1 && d->hidden_dim < 1))
        return fail(GNNB_ERR_INVALID, "feature dims must be positive");
    if (d->num_layers == 0 && d->in_dim != d->out_dim) // models.py:512-518
        return fail(GNNB_ERR_INVALID, "gnn_num_layers=0 needs gnn_output_dim == graph_input_feature_dim");
    if (d->activation < 0 || d->activation > GNNB_ACT_TANH || d->mlp_activation < 0 ||
        d->mlp_activation > GNNB_ACT_TANH)
        return fail(GNNB_ERR_INVALID, "unsupported activation"); // models.py:362
    if (d->num_pools < 1 || d->num_pools > 3)
        return fail(GNNB_ERR_INVALID, "num_pools must be 1..3"); // models.py:332-333
    for (int i = 0; i < d->num_pools; i++)
        if (d->pools[i] < 0 || d->pools[i] > GNNB_POOL_MAX)
            return fail(GNNB_ERR_INVALID, "unsupported pooling %d", d->pools[i]);
    if (d->mlp_num_linear < 1 || d->mlp_num_linear > GNNB_MAX_LAYERS || d->mlp_out < 1 ||
        (d->mlp_num_linear > 1 && d->mlp_hidden < 1))
        return fail(GNNB_ERR_INVALID, "bad MLP head shape");
    if (d->conv_type == GNNB_CONV_PNA && !(d->pna_delta > 0.0f))
        return fail(GNNB_ERR_INVALID, "pna_delta must be > 0");
    if (d->output_activation < GNNB_OUT_NONE || d->output_activation > GNNB_OUT_LOG_SOFTMAX)
        return fail(GNNB_ERR_INVALID, "unsupported output_activation %d", d->output_activation);
    if (d->fpx_w != 0 && (d->fpx_w < 2 || d->fpx_w > 32 || d->fpx_i < 1 || d->fpx_i > 33 || d->fpx_i > d->fpx_w ||
                          d->fpx_w - d->fpx_i > 24))
        return fail(GNNB_ERR_INVALID, "fixed-point emulation takes 2 <= W <= 32, 1 <= I <= W, W - I <= 24 (fp32 carries the "
                                      "grid values exactly only up to 24 fractional bits)");
    if (d->math < -1 || d->math > 3)
        return fail(GNNB_ERR_INVALID, "math must be -1 (follow the process-wide option) or 0 .. 3 (fp32, bf16x6, bf16x3, f16x3)");
    return GNNB_OK;
}

HeadArgs gnnb::model_head_args(const gnnb_model *model)
{
    const gnnb_model_desc &d = model->desc;
    HeadArgs head;
    memset(&head, 0, sizeof(head));
    head.nlin = d.mlp_num_linear;
    for (int i = 0; i < head.nlin && i < 8; i++) {
        int din, dout;
        mlp_dims(d, i, &din, &dout);
        head.w[i] = model->head_w[i];
        head.b[i] = model->head_b[i];
        head.dims[i] = din;
        head.dims[i + 1] = dout;
    }
    return head;
}

namespace {

// host staging image of the blob: every tensor padded to a 16-byte boundary
struct WeightImage {
    std::vector<float> img;
    bool fpx;
    float q_inv, q_step, q_span, q_half;
    explicit WeightImage(const gnnb_model_desc &d)
        : fpx(d.fpx_w > 0), q_inv(fpx ? ldexpf(1.0f, d.fpx_w - d.fpx_i) : 1.0f), q_step(fpx ? ldexpf(1.0f, -(d.fpx_w - d.fpx_i)) : 1.0f),
          q_span(fpx ? ldexpf(1.0f, d.fpx_i) : 1.0f), q_half(fpx ? ldexpf(1.0f, d.fpx_i - 1) : 1.0f)
    {
    }
    size_t push(const float *src, size_t n) // -> offset of the tensor in the image
    {
        size_t off = img.size();
        img.insert(img.end(), src, src + n);
        if (fpx) // W_TYPE = ap_fixed<W, I>: the weights live on the grid (model.h.jinja:41-45)
            for (size_t i = off; i < off + n; i++) {
                float v = floorf(img[i] * q_inv) * q_step;
                img[i] = v - q_span * floorf((v + q_half) / q_span);
            }
        while (img.size() % 4)
            img.push_back(0.0f);
        return off;
    }
    size_t push(const std::vector<float> &v) { return push(v.data(), v.size()); }
};

struct WeightBias { // a derived matrix and the bias that goes with it
    std::vector<float> w, b;
};

// GraphSAGE: lin_l and lin_r fused into one [out, 2*in] matrix [Wl | Wr]; plus_identity: [Wl | Wr + I], the layer's skip
// connection folded into the root weights
std::vector<float> sage_cat_weights(const float *wl, const float *wr, size_t fo, size_t fi, bool plus_identity)
{
    std::vector<float> cat(fo * 2 * fi);
    for (size_t o = 0; o < fo; o++) {
        memcpy(&cat[o * 2 * fi], wl + o * fi, fi * sizeof(float));
        memcpy(&cat[o * 2 * fi + fi], wr + o * fi, fi * sizeof(float));
    }
    if (plus_identity)
        for (size_t o = 0; o < fo; o++)
            cat[o * 2 * fi + fi + o] += 1.0f;
    return cat;
}

// PNA: `lin` folded into the post-NN.  PNAConv applies them back to back with nothing in between
// (out = W_lin (W_post [x | S] + b_post) + b_lin, gnn_builder_lib.h:2081-2157), so
// W' = W_lin W_post [out, 13 F] and b' = W_lin b_post + b_lin (formed in double, rounded once) give the layer
// in ONE 13F-wide GEMM whose epilogue carries the skip operand and the activation: the out x out GEMM and the
// [N, out] hand-over between the two are gone (3 x ~55 us of a BASELINE config 4 step).  Not under the
// fixed-point emulation: the folded matrix is not on the weight grid.
// p = the layer's canonical tensors {W_pre, b_pre, W_post, b_post, W_lin, b_lin}
WeightBias pna_fold_lin(const float *const *p, size_t fi, size_t fo, bool skip_fold)
{
    const size_t K13 = 13 * fi;
    std::vector<double> acc(K13);
    WeightBias f{std::vector<float>(fo * K13), std::vector<float>(fo)};
    for (size_t o = 0; o < fo; o++) {
        std::fill(acc.begin(), acc.end(), 0.0);
        double ab = (double)p[5][o];
        for (size_t h = 0; h < fo; h++) {
            const double wl = (double)p[4][o * fo + h];
            const float *wp = p[2] + h * K13;
            for (size_t k = 0; k < K13; k++)
                acc[k] += wl * (double)wp[k];
            ab += wl * (double)p[3][h];
        }
        if (skip_fold)
            acc[o] += 1.0; // (+ I on the x segment: the skip connection)
        for (size_t k = 0; k < K13; k++)
            f.w[o * K13 + k] = (float)acc[k];
        f.b[o] = (float)ab;
    }
    return f;
}

// PNA, the degree-class form (gnnb_workspace_set_max_degree): for every in-degree c = 0 .. 15 the matrix
//   ( W'_x + S_c Wq | W'_1 + amp W'_2 + att W'_3 ),  [out, 5 F],   and the bias  b' + S_c bq,
// of the folded W' above (`folded`); amp / att as graph prep computes them (k_prep.hip: logf(d + 1) / delta and its
// reciprocal, d = max(c, 1)).  S_c = the max + min + mean column blocks of the class's A matrix: the
// destination's own pre-NN term q_i = Wq x_i + bq shifts max, min and mean of its messages by q_i and
// leaves std alone (gnn_builder_lib.h:1801-1850), so it is folded into x's weights too and the q GEMM is
// not run at all.  Class 0 (no messages: the four aggregates are 0, not q) carries no S term.
// wq = W_pre [F, 2F]: columns [0, F) act on the destination x_i (lib:1801-1802), bias bq
WeightBias pna_degree_class_weights(const WeightBias &folded, const float *wq, const float *bq, size_t fi, size_t fo, float pna_delta)
{
    const size_t K13 = 13 * fi, K5 = 5 * fi;
    WeightBias c5{std::vector<float>((size_t)GNNB_DEG_CLASSES * fo * K5), std::vector<float>((size_t)GNNB_DEG_CLASSES * fo)};
    std::vector<double> wa(4 * fi), sq(fi), sqw(fi);
    for (int c = 0; c < GNNB_DEG_CLASSES; c++) {
        const float lg = logf((float)std::max(c, 1) + 1.0f);
        const double amp = (double)(lg / pna_delta), att = (double)(pna_delta / lg);
        float *dst = &c5.w[(size_t)c * fo * K5];
        for (size_t o = 0; o < fo; o++) {
            const float *src = &folded.w[o * K13];
            for (size_t k = 0; k < 4 * fi; k++)
                wa[k] = (double)src[fi + k] + amp * (double)src[5 * fi + k] + att * (double)src[9 * fi + k];
            for (size_t k = 0; k < 4 * fi; k++)
                dst[o * K5 + fi + k] = (float)wa[k];
            double bsum = (double)folded.b[o];
            if (c > 0) {
                for (size_t k = 0; k < fi; k++)
                    sq[k] = wa[k] + wa[fi + k] + wa[2 * fi + k]; // S_c[o][k]: max + min + mean
                // (S_c Wq)[o][j] = sum_k S_c[o][k] Wq[k][j], k ascending from src[j] as before, but walked
                // along Wq's rows: the column walk (stride 2F) made a 1024-wide PNA layer's upload ~80 s
                for (size_t j = 0; j < fi; j++)
                    sqw[j] = (double)src[j];
                for (size_t k = 0; k < fi; k++) {
                    const double s = sq[k];
                    const float *wr = wq + k * 2 * fi;
                    for (size_t j = 0; j < fi; j++)
                        sqw[j] += s * (double)wr[j];
                }
                for (size_t j = 0; j < fi; j++)
                    dst[o * K5 + j] = (float)sqw[j];
                for (size_t k = 0; k < fi; k++)
                    bsum += sq[k] * (double)bq[k];
            } else {
                for (size_t j = 0; j < fi; j++)
                    dst[o * K5 + j] = src[j];
            }
            c5.b[(size_t)c * fo + o] = (float)bsum;
        }
    }
    return c5;
}

// k_gcn2_zf reads its 16-column slice of the last GCN layer's weight as MFMA B fragments: lane (li, lg) of the wave that
// owns slice s takes W[16 s + li][16 q + 4 lg .. + 3] for q = 0 .. K/16 - 1.  Straight from the [out][in] matrix that is
// 16 rows x 64 B per load instruction (half of every 128-B line unused, 32 MB of L2 traffic per launch over the chip);
// a second copy in fragment order -- float4 index ((s K/16 + q) 4 + lg) 16 + li -- makes every load instruction one
// contiguous KiB.  Rows past `out` are zero.  w1 [out_dim, K]
std::vector<float> zf_fragment_order(const float *w1, int K, int out_dim)
{
    const int KQ = K / 16, NS = (out_dim + 15) / 16;
    std::vector<float> frag((size_t)NS * 16 * K, 0.0f);
    for (int s = 0; s < NS; s++)
        for (int q = 0; q < KQ; q++)
            for (int lg = 0; lg < 4; lg++)
                for (int li = 0; li < 16; li++) {
                    const int n = 16 * s + li;
                    if (n >= out_dim)
                        continue;
                    for (int e = 0; e < 4; e++)
                        frag[((((size_t)s * KQ + q) * 4 + lg) * 16 + li) * 4 + e] = w1[(size_t)n * K + 16 * q + 4 * lg + e];
                }
    return frag;
}

// GIN stacks: every wide matrix once more in EXECUTION order at one hidden x hidden stride, zero-padded (gnnb_model::gin_w):
// index 0 = layer 0's second linear, 2l - 1 / 2l = layer l's first / second linear; the biases likewise.  Read from the
// image (conv_off: the layers' canonical slots in it), so the copies are on the fixed-point grid when the originals are.
WeightBias gin_execution_order(const gnnb_model_desc &d, const std::vector<float> &img, const std::vector<std::vector<size_t>> &conv_off)
{
    const size_t h = d.hidden_dim, ho = d.out_dim;
    const int L = d.num_layers, nm = 2 * L - 1;
    WeightBias g{std::vector<float>((size_t)nm * h * h, 0.0f), std::vector<float>((size_t)nm * h, 0.0f)};
    auto put = [&](int idx, size_t off_w, size_t off_b, size_t rows, size_t cols) { // [rows, cols] -> top-left of slot idx
        for (size_t r = 0; r < rows; r++)
            memcpy(&g.w[(size_t)idx * h * h + r * h], &img[off_w + r * cols], cols * sizeof(float));
        memcpy(&g.b[(size_t)idx * h], &img[off_b], rows * sizeof(float));
    };
    put(0, conv_off[0][2], conv_off[0][3], L == 1 ? ho : h, L == 1 ? ho : h); // (layer 0's second linear)
    for (int l = 1; l < L; l++) {
        const size_t fo = l == L - 1 ? ho : h;
        put(2 * l - 1, conv_off[l][0], conv_off[l][1], fo, h); // Wa [fo, h]
        put(2 * l, conv_off[l][2], conv_off[l][3], fo, fo);     // Wb [fo, fo]
    }
    return g;
}

// One conv layer's canonical tensors p[] and, behind them, the derived slots its conv type has -> their offsets in the image
// edge_dim > 0 (a GINE model: GIN's four tensors, then conv.lin): slots 4, 5 = W_e [in, edge_dim], b_e [in]
std::vector<size_t> push_conv_layer(WeightImage &im, const gnnb_model_desc &d, int l, const float *const *p, int edge_dim)
{
    const LayerDims ld = layer_dims(d, l);
    const size_t fi = ld.fin, fo = ld.fout;
    // the layer's skip connection (middle layers: y = conv(x) + x, models.py:562-564) where x itself is an operand of
    // the layer's GEMM (GraphSAGE's root term, PNA's x segment): folded into that operand's weights as + I, so that the
    // [N, out] skip operand is not read again in the epilogue (45 of 293 us of a 128-wide PNA layer's GEMM went there:
    // 32-byte pieces of 128-byte lines)
    const bool skip_fold = d.skip && l != 0 && l != d.num_layers - 1 && fi == fo && !im.fpx;
    std::vector<size_t> off;
    switch (d.conv_type) {
    case GNNB_CONV_GCN:
        off = {im.push(p[0], fo * fi), im.push(p[1], fo)};
        break;
    case GNNB_CONV_GIN: // hidden = out_channels (models.py:90)
        off = {im.push(p[0], fo * fi), im.push(p[1], fo), im.push(p[2], fo * fo), im.push(p[3], fo)};
        if (edge_dim > 0) {
            off.push_back(im.push(p[4], fi * (size_t)edge_dim));
            off.push_back(im.push(p[5], fi));
        }
        break;
    case GNNB_CONV_SAGE:
        off = {im.push(sage_cat_weights(p[0], p[2], fo, fi, false)), im.push(p[1], fo)};
        if (skip_fold) // slot 2: [Wl | Wr + I]
            off.push_back(im.push(sage_cat_weights(p[0], p[2], fo, fi, true)));
        break;
    case GNNB_CONV_PNA:
        off = {im.push(p[0], fi * 2 * fi), im.push(p[1], fi), im.push(p[2], fo * 13 * fi),
               im.push(p[3], fo),          im.push(p[4], fo * fo), im.push(p[5], fo)};
        if (!im.fpx) {
            const WeightBias folded = pna_fold_lin(p, fi, fo, skip_fold); // slots 6, 7
            off.push_back(im.push(folded.w));
            off.push_back(im.push(folded.b));
            if (fo > 32) { // slots 8, 9 (any input width: whole 32-wide chunks take k_linear_dma's row-class mode, others the generic kernel's)
                const WeightBias classes = pna_degree_class_weights(folded, p[0], p[1], fi, fo, d.pna_delta);
                off.push_back(im.push(classes.w));
                off.push_back(im.push(classes.b));
            }
        }
        break;
    }
    return off;
}

// parameter tensors of a model; edge_dim > 0: a GINE model (two more per conv layer), which GIN descriptions without the
// fixed-point emulation have
int count_params(const gnnb_model_desc *desc, int edge_dim)
{
    int rc = validate_desc(desc);
    if (rc != GNNB_OK)
        return rc;
    if (edge_dim != 0) {
        if (edge_dim < 1 || edge_dim > 16)
            return fail(GNNB_ERR_INVALID, "edge_dim %d: a GINE model takes 1 .. 16 edge attributes", edge_dim);
        if (desc->conv_type != GNNB_CONV_GIN)
            return fail(GNNB_ERR_INVALID, "a GINE model's description is a GIN description (conv_type %d given)", desc->conv_type);
        if (desc->fpx_w != 0)
            return fail(GNNB_ERR_INVALID, "the fixed-point emulation does not cover GINE models (fpx_w must be 0)");
    }
    return (conv_slots(desc->conv_type) + (edge_dim ? 2 : 0)) * desc->num_layers + 2 * desc->mlp_num_linear;
}

// gnnb_model_create and gnnb_edge_model_create (edge_dim > 0)
int model_create(const gnnb_model_desc *desc, int edge_dim, const float *const *host_params, int num_params, gnnb_model **out_model)
{
    if (!out_model)
        return fail(GNNB_ERR_INVALID, "null out_model");
    *out_model = nullptr;
    int expect = count_params(desc, edge_dim);
    if (expect < 0)
        return expect;
    if (num_params != expect || !host_params)
        return fail(GNNB_ERR_INVALID, "expected %d parameter tensors, got %d", expect, num_params);
    for (int i = 0; i < num_params; i++)
        if (!host_params[i])
            return fail(GNNB_ERR_INVALID, "parameter %d is NULL", i);
    if (gnnb_device_count() <= 0)
        return fail(GNNB_ERR_NO_DEVICE, "no HIP device visible: the MI355X path cannot run");

    // the image, in blob order: conv layers (canonical + derived slots), k_gcn2_zf's fragment copy, the GIN stack's copies, the head
    const gnnb_model_desc &d = *desc;
    WeightImage im(d);
    std::vector<std::vector<size_t>> conv_off(d.num_layers);
    const int slots = conv_slots(d.conv_type) + (edge_dim ? 2 : 0);
    int pi = 0;
    for (int l = 0; l < d.num_layers; l++, pi += slots)
        conv_off[l] = push_conv_layer(im, d, l, host_params + pi, edge_dim);
    size_t w1f_off = 0;
    const bool have_w1f = d.conv_type == GNNB_CONV_GCN && d.num_layers == 2 && d.hidden_dim % 16 == 0 && d.hidden_dim <= 128 && d.out_dim <= 128;
    if (have_w1f) // (from the image copy: already on the fixed-point grid when fpx is set; push() quantising again is harmless -- the grid is idempotent)
        w1f_off = im.push(zf_fragment_order(&im.img[conv_off[1][0]], d.hidden_dim, d.out_dim));
    size_t gin_w_off = 0, gin_b_off = 0;
    // (a GINE model takes no stack kernel: no execution-order copy)
    const bool have_gin = edge_dim == 0 && d.conv_type == GNNB_CONV_GIN && d.num_layers >= 2 && (d.hidden_dim == 32 || d.hidden_dim == 64 || d.hidden_dim == 128) &&
                          d.out_dim <= d.hidden_dim && d.out_dim % 4 == 0;
    if (have_gin) {
        const WeightBias g = gin_execution_order(d, im.img, conv_off);
        gin_w_off = im.push(g.w);
        gin_b_off = im.push(g.b);
    }
    std::vector<size_t> hw, hb;
    for (int i = 0; i < d.mlp_num_linear; i++, pi += 2) {
        int din, dout;
        mlp_dims(d, i, &din, &dout);
        hw.push_back(im.push(host_params[pi], (size_t)din * dout));
        hb.push_back(im.push(host_params[pi + 1], (size_t)dout));
    }
    const std::vector<float> &img = im.img;

    gnnb_model *m = new gnnb_model();
    m->desc = d;
    m->edge_dim = edge_dim;
    (void)hipGetDevice(&m->device);
    m->blob_floats = img.size();
    hipError_t e = hipMalloc((void **)&m->blob, std::max<size_t>(img.size(), 4) * sizeof(float));
    if (e == hipSuccess && !img.empty())
        e = hipMemcpy(m->blob, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (m->blob)
            (void)hipFree(m->blob);
        delete m;
        return fail(GNNB_ERR_HIP, "weight upload failed: %s", hipGetErrorString(e));
    }
    m->conv.resize(d.num_layers);
    for (int l = 0; l < d.num_layers; l++)
        for (size_t off : conv_off[l])
            m->conv[l].push_back(m->blob + off);
    if (have_w1f)
        m->zf_w1f = m->blob + w1f_off;
    if (have_gin) {
        m->gin_w = m->blob + gin_w_off;
        m->gin_b = m->blob + gin_b_off;
    }
    for (int i = 0; i < d.mlp_num_linear; i++) {
        m->head_w.push_back(m->blob + hw[i]);
        m->head_b.push_back(m->blob + hb[i]);
    }
    if (d.mlp_num_linear <= 8) { // (best effort: without the device copy the stack kernels leave the head to its own launch)
        const HeadArgs h = model_head_args(m);
        if (hipMalloc((void **)&m->head_dev, sizeof(HeadArgs)) != hipSuccess ||
            hipMemcpy(m->head_dev, &h, sizeof(HeadArgs), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError();
            if (m->head_dev)
                (void)hipFree(m->head_dev);
            m->head_dev = nullptr;
        }
    }
    *out_model = m;
    return GNNB_OK;
}

} // namespace

extern "C" {

int gnnb_model_num_params(const gnnb_model_desc *desc) { return count_params(desc, 0); }

int gnnb_model_create(const gnnb_model_desc *desc, const float *const *host_params, int num_params, gnnb_model **out_model)
{
    return model_create(desc, 0, host_params, num_params, out_model);
}

int gnnb_edge_model_num_params(const gnnb_model_desc *desc, int edge_dim)
{
    if (edge_dim == 0)
        return fail(GNNB_ERR_INVALID, "edge_dim 0: a GINE model takes 1 .. 16 edge attributes (gnnb_model_num_params: models without)");
    return count_params(desc, edge_dim);
}

int gnnb_edge_model_create(const gnnb_model_desc *desc, int edge_dim, const float *const *host_params, int num_params,
                           gnnb_model **out_model)
{
    if (out_model)
        *out_model = nullptr;
    if (edge_dim == 0)
        return fail(GNNB_ERR_INVALID, "edge_dim 0: a GINE model takes 1 .. 16 edge attributes (gnnb_model_create: models without)");
    return model_create(desc, edge_dim, host_params, num_params, out_model);
}

int gnnb_model_edge_dim(const gnnb_model *model) { return model ? model->edge_dim : 0; }

void gnnb_model_destroy(gnnb_model *model)
{
    if (!model)
        return;
    if (model->blob)
        (void)hipFree(model->blob);
    if (model->head_dev)
        (void)hipFree(model->head_dev);
    delete model;
}

int gnnb_model_get_desc(const gnnb_model *model, gnnb_model_desc *out_desc)
{
    if (!model || !out_desc)
        return fail(GNNB_ERR_INVALID, "null argument");
    *out_desc = model->desc;
    return GNNB_OK;
}

} // extern "C"
