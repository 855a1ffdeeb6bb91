// gnnb_model.hip -- the model handle of libgnnb_hip.so: validation of a description, and gnnb_model_create's weight upload --
// the image build_weight_image lays out (gnnb_weights.h: the canonical tensors plus the derived forms the kernels read) as ONE
// device blob, its offsets turned into the model's pointers.
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

// the model's two device allocations: freed here for gnnb_model_destroy and for a failed gnnb_model_create alike
gnnb_model::~gnnb_model()
{
    if (blob)
        (void)hipFree(blob);
    if (head_dev)
        (void)hipFree(head_dev);
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

// parameter tensors of a model; edge_dim > 0: an edge model (two more per conv layer), which descriptions of conv type `base` --
// GIN: a GINE model (gnnb_edge.h), PNA: PNA with edge features (gnnb_pna_edge.h) -- without the fixed-point emulation have
int count_params(const gnnb_model_desc *desc, int edge_dim, int base = GNNB_CONV_GIN)
{
    int rc = validate_desc(desc);
    if (rc != GNNB_OK)
        return rc;
    if (edge_dim != 0) {
        const char *const kind = base == GNNB_CONV_PNA ? "PNA edge" : "GINE";
        if (edge_dim < 1 || edge_dim > 16)
            return fail(GNNB_ERR_INVALID, "edge_dim %d: a %s model takes 1 .. 16 edge attributes", edge_dim, kind);
        if (desc->conv_type != base)
            return fail(GNNB_ERR_INVALID, "a %s model's description is a %s description (conv_type %d given)", kind,
                        base == GNNB_CONV_PNA ? "PNA" : "GIN", desc->conv_type);
        if (desc->fpx_w != 0)
            return fail(GNNB_ERR_INVALID, "the fixed-point emulation does not cover %s models (fpx_w must be 0)", kind);
    }
    return (conv_slots(desc->conv_type) + (edge_dim ? 2 : 0)) * desc->num_layers + 2 * desc->mlp_num_linear;
}

// parameter tensors of a GATv2 model (gnnb_gat.h): a GCN description without the fixed-point emulation, heads 1 .. 8 dividing every
// layer's output width, which is at most 256; edge_dim != 0: with edge features (gnnb_gat_edge.h), 1 .. 16, one more tensor per layer
int count_gat_params(const gnnb_model_desc *desc, int heads, int edge_dim = 0)
{
    int rc = validate_desc(desc);
    if (rc != GNNB_OK)
        return rc;
    if (heads < 1 || heads > GAT_MAX_HEADS)
        return fail(GNNB_ERR_INVALID, "heads %d: a GATv2 model takes 1 .. %d heads", heads, GAT_MAX_HEADS);
    if (edge_dim != 0 && (edge_dim < 1 || edge_dim > 16))
        return fail(GNNB_ERR_INVALID, "edge_dim %d: a GATv2 model with edge features takes 1 .. 16 edge attributes", edge_dim);
    if (desc->conv_type != GNNB_CONV_GCN)
        return fail(GNNB_ERR_INVALID, "a GATv2 model's description is a GCN description (conv_type %d given)", desc->conv_type);
    if (desc->fpx_w != 0)
        return fail(GNNB_ERR_INVALID, "the fixed-point emulation does not cover GATv2 models (fpx_w must be 0)");
    for (int l = 0; l < desc->num_layers; l++) {
        const int fo = layer_dims(*desc, l).fout;
        if (fo % heads != 0)
            return fail(GNNB_ERR_INVALID, "layer %d's output width %d is not divisible by heads %d", l, fo, heads);
        if (fo > GAT_MAX_WIDTH)
            return fail(GNNB_ERR_INVALID, "layer %d's output width %d: a GATv2 layer is at most %d wide", l, fo, GAT_MAX_WIDTH);
    }
    return (GAT_PARAM_SLOTS + (edge_dim ? 1 : 0)) * desc->num_layers + 2 * desc->mlp_num_linear;
}

// parameter tensors of a GAT v1 model (gnnb_gatconv.h): GATv2's conditions on the description and on heads; four tensors per layer
// (edge_dim != 0: with edge features, gnnb_gatconv_edge.h, 1 .. 16 -- att_edge and lin_edge's weight are two more per layer)
int count_gatconv_params(const gnnb_model_desc *desc, int heads, int edge_dim = 0)
{
    int rc = validate_desc(desc);
    if (rc != GNNB_OK)
        return rc;
    if (heads < 1 || heads > GAT_MAX_HEADS)
        return fail(GNNB_ERR_INVALID, "heads %d: a GAT model takes 1 .. %d heads", heads, GAT_MAX_HEADS);
    if (edge_dim != 0 && (edge_dim < 1 || edge_dim > 16))
        return fail(GNNB_ERR_INVALID, "edge_dim %d: a GAT model with edge features takes 1 .. 16 edge attributes", edge_dim);
    if (desc->conv_type != GNNB_CONV_GCN)
        return fail(GNNB_ERR_INVALID, "a GAT model's description is a GCN description (conv_type %d given)", desc->conv_type);
    if (desc->fpx_w != 0)
        return fail(GNNB_ERR_INVALID, "the fixed-point emulation does not cover GAT models (fpx_w must be 0)");
    for (int l = 0; l < desc->num_layers; l++) {
        const int fo = layer_dims(*desc, l).fout;
        if (fo % heads != 0)
            return fail(GNNB_ERR_INVALID, "layer %d's output width %d is not divisible by heads %d", l, fo, heads);
        if (fo > GAT_MAX_WIDTH)
            return fail(GNNB_ERR_INVALID, "layer %d's output width %d: a GAT layer is at most %d wide", l, fo, GAT_MAX_WIDTH);
    }
    return (GAT1_PARAM_SLOTS + (edge_dim ? 2 : 0)) * desc->num_layers + 2 * desc->mlp_num_linear;
}

// parameter tensors of a TransformerConv model (gnnb_transformer.h): a GIN description (its tables keep explicit (v, v) edges) without
// the fixed-point emulation, heads 1 .. 8 dividing every layer's output width, which is at most 256
// (edge_dim != 0: with edge features, gnnb_transformer_edge.h -- lin_edge's weight is a ninth tensor per layer)
int count_transformer_params(const gnnb_model_desc *desc, int heads, int edge_dim = 0)
{
    int rc = validate_desc(desc);
    if (rc != GNNB_OK)
        return rc;
    if (heads < 1 || heads > TF_MAX_HEADS)
        return fail(GNNB_ERR_INVALID, "heads %d: a TransformerConv model takes 1 .. %d heads", heads, TF_MAX_HEADS);
    if (desc->conv_type != GNNB_CONV_GIN)
        return fail(GNNB_ERR_INVALID, "a TransformerConv model's description is a GIN description (conv_type %d given)", desc->conv_type);
    if (desc->fpx_w != 0)
        return fail(GNNB_ERR_INVALID, "the fixed-point emulation does not cover TransformerConv models (fpx_w must be 0)");
    for (int l = 0; l < desc->num_layers; l++) {
        const int fo = layer_dims(*desc, l).fout;
        if (fo % heads != 0)
            return fail(GNNB_ERR_INVALID, "layer %d's output width %d is not divisible by heads %d", l, fo, heads);
        if (fo > TF_MAX_WIDTH)
            return fail(GNNB_ERR_INVALID, "layer %d's output width %d: a TransformerConv layer is at most %d wide", l, fo, TF_MAX_WIDTH);
    }
    if (edge_dim != 0 && (edge_dim < 1 || edge_dim > TFE_MAX_EDGE_DIM))
        return fail(GNNB_ERR_INVALID, "edge_dim %d: a TransformerConv model with edge features takes edge_dim 1 .. %d", edge_dim,
                    TFE_MAX_EDGE_DIM);
    return (TF_PARAM_SLOTS + (edge_dim ? 1 : 0)) * desc->num_layers + 2 * desc->mlp_num_linear;
}

// parameter tensors of a ResGatedGraphConv model (gnnb_resgated.h): a GIN description (its tables keep explicit (v, v) edges) without
// the fixed-point emulation, every layer's output width at most 256 (edge_dim != 0: with edge features, gnnb_resgated_edge.h -- the
// same eight tensors per layer, lin_key / lin_query / lin_value [out, in + edge_dim])
int count_resgated_params(const gnnb_model_desc *desc, int edge_dim = 0)
{
    int rc = validate_desc(desc);
    if (rc != GNNB_OK)
        return rc;
    if (edge_dim != 0 && (edge_dim < 1 || edge_dim > RGE_MAX_EDGE_DIM))
        return fail(GNNB_ERR_INVALID, "edge_dim %d: a ResGatedGraphConv model with edge features takes edge_dim 1 .. %d", edge_dim,
                    RGE_MAX_EDGE_DIM);
    if (desc->conv_type != GNNB_CONV_GIN)
        return fail(GNNB_ERR_INVALID, "a ResGatedGraphConv model's description is a GIN description (conv_type %d given)", desc->conv_type);
    if (desc->fpx_w != 0)
        return fail(GNNB_ERR_INVALID, "the fixed-point emulation does not cover ResGatedGraphConv models (fpx_w must be 0)");
    for (int l = 0; l < desc->num_layers; l++) {
        const int fo = layer_dims(*desc, l).fout;
        if (fo > RG_MAX_WIDTH)
            return fail(GNNB_ERR_INVALID, "layer %d's output width %d: a ResGatedGraphConv layer is at most %d wide", l, fo, RG_MAX_WIDTH);
    }
    return RG_PARAM_SLOTS * desc->num_layers + 2 * desc->mlp_num_linear;
}

// parameter tensors of a GatedGraphConv model (gnnb_ggnn.h): a GIN description (its tables keep explicit (v, v) edges) without the
// fixed-point emulation, steps 1 .. 8, every layer's input width at most its output width (h_0 = [x | 0]), which is at most 256
int count_ggnn_params(const gnnb_model_desc *desc, int steps)
{
    int rc = validate_desc(desc);
    if (rc != GNNB_OK)
        return rc;
    if (steps < 1 || steps > GGNN_MAX_STEPS)
        return fail(GNNB_ERR_INVALID, "steps %d: a GatedGraphConv model takes 1 .. %d steps per layer", steps, GGNN_MAX_STEPS);
    if (desc->conv_type != GNNB_CONV_GIN)
        return fail(GNNB_ERR_INVALID, "a GatedGraphConv model's description is a GIN description (conv_type %d given)", desc->conv_type);
    if (desc->fpx_w != 0)
        return fail(GNNB_ERR_INVALID, "the fixed-point emulation does not cover GatedGraphConv models (fpx_w must be 0)");
    for (int l = 0; l < desc->num_layers; l++) {
        const LayerDims ld = layer_dims(*desc, l);
        if (ld.fin > ld.fout)
            return fail(GNNB_ERR_INVALID, "layer %d's input width %d exceeds its output width %d: a GatedGraphConv layer pads its input with "
                                          "zero columns and cannot narrow it", l, ld.fin, ld.fout);
        if (ld.fout > GG_MAX_WIDTH)
            return fail(GNNB_ERR_INVALID, "layer %d's output width %d: a GatedGraphConv layer is at most %d wide", l, ld.fout, GG_MAX_WIDTH);
    }
    return GGNN_PARAM_SLOTS * desc->num_layers + 2 * desc->mlp_num_linear;
}

// parameter tensors of an RGCNConv model (gnnb_rgcn.h): a GIN description (its tables keep explicit (v, v) edges) without the
// fixed-point emulation, relations 1 .. 8, every layer's output width at most 256
int count_rgcn_params(const gnnb_model_desc *desc, int relations)
{
    int rc = validate_desc(desc);
    if (rc != GNNB_OK)
        return rc;
    if (relations < 1 || relations > RGCN_MAX_RELATIONS)
        return fail(GNNB_ERR_INVALID, "relations %d: an RGCNConv model takes 1 .. %d relations", relations, RGCN_MAX_RELATIONS);
    if (desc->conv_type != GNNB_CONV_GIN)
        return fail(GNNB_ERR_INVALID, "an RGCNConv model's description is a GIN description (conv_type %d given)", desc->conv_type);
    if (desc->fpx_w != 0)
        return fail(GNNB_ERR_INVALID, "the fixed-point emulation does not cover RGCNConv models (fpx_w must be 0)");
    for (int l = 0; l < desc->num_layers; l++)
        if (layer_dims(*desc, l).fout > RGCN_MAX_WIDTH)
            return fail(GNNB_ERR_INVALID, "layer %d's output width %d: an RGCNConv layer is at most %d wide", l, layer_dims(*desc, l).fout,
                        RGCN_MAX_WIDTH);
    return RGCN_PARAM_SLOTS * desc->num_layers + 2 * desc->mlp_num_linear;
}

// What travels beside a description, by name: nothing (gnnb_model_create), edge_dim of an edge model whose description has conv
// type `base` (gnnb_edge_model_create: GIN, gnnb_pna_edge_model_create: PNA), or heads and negative_slope of a GATv2 model
// (gnnb_gat_model_create: a GCN description), or all three (gnnb_gat_edge_model_create: GATv2 with edge features), or heads of a
// TransformerConv model (gnnb_transformer_model_create: a GIN description), or heads and edge_dim
// (gnnb_transformer_edge_model_create: TransformerConv with edge features), or the "gated" mark of a ResGatedGraphConv model
// (gnnb_resgated_model_create: a GIN description), or that mark and edge_dim (gnnb_resgated_edge_model_create: ResGatedGraphConv with
// edge features), or heads and negative_slope of a GAT v1 model (gnnb_gatconv_model_create: a GCN description), or the steps of a
// GatedGraphConv model (gnnb_ggnn_model_create: a GIN description), or the relations of an RGCNConv model (gnnb_rgcn_model_create: a
// GIN description)
struct ModelKind {
    int edge_dim = 0, base = GNNB_CONV_GIN;
    int gat_heads = 0;
    float gat_slope = 0.0f;
    int tf_heads = 0;
    bool gated = false;
    int gat1_heads = 0; // (its slope: gat_slope)
    int ggnn_steps = 0;
    int rgcn_relations = 0;
    static ModelKind plain() { return {}; }
    static ModelKind edges(int edge_dim, int base)
    {
        ModelKind k;
        k.edge_dim = edge_dim, k.base = base;
        return k;
    }
    static ModelKind gatv2(int heads, float slope)
    {
        ModelKind k;
        k.gat_heads = heads, k.gat_slope = slope;
        return k;
    }
    static ModelKind gatv2_edges(int heads, float slope, int edge_dim)
    {
        ModelKind k = gatv2(heads, slope);
        k.edge_dim = edge_dim, k.base = GNNB_CONV_GCN;
        return k;
    }
    static ModelKind gatconv(int heads, float slope)
    {
        ModelKind k;
        k.gat1_heads = heads, k.gat_slope = slope;
        return k;
    }
    static ModelKind gatconv_edges(int heads, float slope, int edge_dim)
    {
        ModelKind k = gatconv(heads, slope);
        k.edge_dim = edge_dim, k.base = GNNB_CONV_GCN;
        return k;
    }
    static ModelKind transformer(int heads)
    {
        ModelKind k;
        k.tf_heads = heads;
        return k;
    }
    static ModelKind transformer_edges(int heads, int edge_dim)
    {
        ModelKind k = transformer(heads);
        k.edge_dim = edge_dim;
        return k;
    }
    static ModelKind resgated()
    {
        ModelKind k;
        k.gated = true;
        return k;
    }
    static ModelKind ggnn(int steps)
    {
        ModelKind k;
        k.ggnn_steps = steps;
        return k;
    }
    static ModelKind rgcn(int relations)
    {
        ModelKind k;
        k.rgcn_relations = relations;
        return k;
    }
    static ModelKind resgated_edges(int edge_dim)
    {
        ModelKind k = resgated();
        k.edge_dim = edge_dim;
        return k;
    }
};

// the body of the thirteen *_model_create entries
int model_create(const gnnb_model_desc *desc, const ModelKind &kind, const float *const *host_params, int num_params, gnnb_model **out_model)
{
    if (!out_model)
        return fail(GNNB_ERR_INVALID, "null out_model");
    *out_model = nullptr;
    const int edge_dim = kind.edge_dim, gat_heads = kind.gat_heads, tf_heads = kind.tf_heads;
    const int gat1_heads = kind.gat1_heads;
    int expect = kind.rgcn_relations != 0 ? count_rgcn_params(desc, kind.rgcn_relations)
                 : kind.ggnn_steps != 0 ? count_ggnn_params(desc, kind.ggnn_steps)
                 : gat1_heads != 0 ? count_gatconv_params(desc, gat1_heads, edge_dim)
                 : kind.gated     ? count_resgated_params(desc, edge_dim)
                 : tf_heads != 0  ? count_transformer_params(desc, tf_heads, edge_dim)
                 : gat_heads != 0 ? count_gat_params(desc, gat_heads, edge_dim)
                                  : count_params(desc, edge_dim, kind.base);
    if (expect < 0)
        return expect;
    if ((gat_heads != 0 || gat1_heads != 0) && !std::isfinite(kind.gat_slope))
        return fail(GNNB_ERR_INVALID, "negative_slope must be finite");
    if (num_params != expect || !host_params)
        return fail(GNNB_ERR_INVALID, "expected %d parameter tensors, got %d", expect, num_params);
    for (int i = 0; i < num_params; i++)
        if (!host_params[i])
            return fail(GNNB_ERR_INVALID, "parameter %d is NULL", i);
    if (gnnb_device_count() <= 0)
        return fail(GNNB_ERR_NO_DEVICE, "no HIP device visible: the MI355X path cannot run");

    const gnnb_model_desc &d = *desc;
    const BuiltWeights built = build_weight_image(d, edge_dim, host_params, gat_heads, tf_heads, kind.gated, gat1_heads, kind.ggnn_steps, kind.rgcn_relations);
    const std::vector<float> &img = built.img;
    const WeightLayout &lo = built.layout;

    gnnb_model *m = new gnnb_model();
    m->desc = d;
    m->edge_dim = edge_dim;
    m->gat_heads = gat_heads;
    m->gat_slope = gat_heads || gat1_heads ? kind.gat_slope : 0.0f;
    m->gat1_heads = gat1_heads;
    m->tf_heads = tf_heads;
    m->gated = kind.gated ? 1 : 0;
    m->ggnn_steps = kind.ggnn_steps;
    m->rgcn_relations = kind.rgcn_relations;
    (void)hipGetDevice(&m->device);
    m->blob_floats = img.size();
    hipError_t e = hipMalloc((void **)&m->blob, std::max<size_t>(img.size(), 4) * sizeof(float));
    if (e == hipSuccess && !img.empty())
        e = hipMemcpy(m->blob, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        delete m;
        return fail(GNNB_ERR_HIP, "weight upload failed: %s", hipGetErrorString(e));
    }
    const float *const blob = m->blob;
    auto at = [blob](size_t off) { return off == NO_OFFSET ? (const float *)nullptr : blob + off; }; // an offset of the layout -> its device pointer
    for (const LayerOffsets &l : lo.conv)
        m->conv.push_back(l.map(at));
    m->zf_w1f = at(lo.zf_w1f);
    m->gin_w = at(lo.gin_w);
    m->gin_b = at(lo.gin_b);
    for (int i = 0; i < d.mlp_num_linear; i++) {
        m->head_w.push_back(at(lo.head_w[i]));
        m->head_b.push_back(at(lo.head_b[i]));
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
    return model_create(desc, ModelKind::plain(), host_params, num_params, out_model);
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
    return model_create(desc, ModelKind::edges(edge_dim, GNNB_CONV_GIN), host_params, num_params, out_model);
}

int gnnb_pna_edge_model_num_params(const gnnb_model_desc *desc, int edge_dim)
{
    if (edge_dim == 0)
        return fail(GNNB_ERR_INVALID, "edge_dim 0: a PNA edge model takes 1 .. 16 edge attributes (gnnb_model_num_params: models without)");
    return count_params(desc, edge_dim, GNNB_CONV_PNA);
}

int gnnb_pna_edge_model_create(const gnnb_model_desc *desc, int edge_dim, const float *const *host_params, int num_params,
                               gnnb_model **out_model)
{
    if (out_model)
        *out_model = nullptr;
    if (edge_dim == 0)
        return fail(GNNB_ERR_INVALID, "edge_dim 0: a PNA edge model takes 1 .. 16 edge attributes (gnnb_model_create: models without)");
    return model_create(desc, ModelKind::edges(edge_dim, GNNB_CONV_PNA), host_params, num_params, out_model);
}

int gnnb_model_edge_dim(const gnnb_model *model) { return model ? model->edge_dim : 0; }

int gnnb_gat_model_num_params(const gnnb_model_desc *desc, int heads) { return count_gat_params(desc, heads); }

int gnnb_gat_model_create(const gnnb_model_desc *desc, int heads, float negative_slope, const float *const *host_params, int num_params,
                          gnnb_model **out_model)
{
    if (out_model)
        *out_model = nullptr;
    if (heads == 0) // (ModelKind reads 0 as "no GATv2 model")
        return fail(GNNB_ERR_INVALID, "heads 0: a GATv2 model takes 1 .. %d heads", GAT_MAX_HEADS);
    return model_create(desc, ModelKind::gatv2(heads, negative_slope), host_params, num_params, out_model);
}

int gnnb_model_gat_heads(const gnnb_model *model) { return model ? model->gat_heads : 0; }

int gnnb_gat_edge_model_num_params(const gnnb_model_desc *desc, int heads, int edge_dim)
{
    if (edge_dim == 0)
        return fail(GNNB_ERR_INVALID, "edge_dim 0: a GATv2 model with edge features takes 1 .. 16 edge attributes (gnnb_gat_model_num_params: "
                                      "models without)");
    return count_gat_params(desc, heads, edge_dim);
}

int gnnb_gat_edge_model_create(const gnnb_model_desc *desc, int heads, float negative_slope, int edge_dim, const float *const *host_params,
                               int num_params, gnnb_model **out_model)
{
    if (out_model)
        *out_model = nullptr;
    if (heads == 0) // (ModelKind reads 0 as "no GATv2 model")
        return fail(GNNB_ERR_INVALID, "heads 0: a GATv2 model takes 1 .. %d heads", GAT_MAX_HEADS);
    if (edge_dim == 0)
        return fail(GNNB_ERR_INVALID, "edge_dim 0: a GATv2 model with edge features takes 1 .. 16 edge attributes (gnnb_gat_model_create: models "
                                      "without)");
    return model_create(desc, ModelKind::gatv2_edges(heads, negative_slope, edge_dim), host_params, num_params, out_model);
}

int gnnb_gatconv_model_num_params(const gnnb_model_desc *desc, int heads) { return count_gatconv_params(desc, heads); }

int gnnb_gatconv_model_create(const gnnb_model_desc *desc, int heads, float negative_slope, const float *const *host_params, int num_params,
                              gnnb_model **out_model)
{
    if (out_model)
        *out_model = nullptr;
    if (heads == 0) // (ModelKind reads 0 as "no GAT model")
        return fail(GNNB_ERR_INVALID, "heads 0: a GAT model takes 1 .. %d heads", GAT_MAX_HEADS);
    return model_create(desc, ModelKind::gatconv(heads, negative_slope), host_params, num_params, out_model);
}

int gnnb_model_gatconv_heads(const gnnb_model *model) { return model ? model->gat1_heads : 0; }

int gnnb_gatconv_edge_model_num_params(const gnnb_model_desc *desc, int heads, int edge_dim)
{
    if (edge_dim == 0)
        return fail(GNNB_ERR_INVALID, "edge_dim 0: a GAT model with edge features takes 1 .. 16 edge attributes (gnnb_gatconv_model_num_params: "
                                      "models without)");
    return count_gatconv_params(desc, heads, edge_dim);
}

int gnnb_gatconv_edge_model_create(const gnnb_model_desc *desc, int heads, float negative_slope, int edge_dim, const float *const *host_params,
                                   int num_params, gnnb_model **out_model)
{
    if (out_model)
        *out_model = nullptr;
    if (heads == 0) // (ModelKind reads 0 as "no GAT model")
        return fail(GNNB_ERR_INVALID, "heads 0: a GAT model takes 1 .. %d heads", GAT_MAX_HEADS);
    if (edge_dim == 0)
        return fail(GNNB_ERR_INVALID, "edge_dim 0: a GAT model with edge features takes 1 .. 16 edge attributes (gnnb_gatconv_model_create: "
                                      "models without)");
    return model_create(desc, ModelKind::gatconv_edges(heads, negative_slope, edge_dim), host_params, num_params, out_model);
}

int gnnb_transformer_model_num_params(const gnnb_model_desc *desc, int heads) { return count_transformer_params(desc, heads); }

int gnnb_transformer_model_create(const gnnb_model_desc *desc, int heads, const float *const *host_params, int num_params,
                                  gnnb_model **out_model)
{
    if (out_model)
        *out_model = nullptr;
    if (heads == 0) // (ModelKind reads 0 as "no TransformerConv model")
        return fail(GNNB_ERR_INVALID, "heads 0: a TransformerConv model takes 1 .. %d heads", TF_MAX_HEADS);
    return model_create(desc, ModelKind::transformer(heads), host_params, num_params, out_model);
}

int gnnb_model_transformer_heads(const gnnb_model *model) { return model ? model->tf_heads : 0; }

int gnnb_transformer_edge_model_num_params(const gnnb_model_desc *desc, int heads, int edge_dim)
{
    if (edge_dim == 0) // (count_transformer_params reads 0 as "no edge features")
        return fail(GNNB_ERR_INVALID, "edge_dim 0: a TransformerConv model with edge features takes edge_dim 1 .. %d", TFE_MAX_EDGE_DIM);
    return count_transformer_params(desc, heads, edge_dim);
}

int gnnb_transformer_edge_model_create(const gnnb_model_desc *desc, int heads, int edge_dim, const float *const *host_params, int num_params,
                                       gnnb_model **out_model)
{
    if (out_model)
        *out_model = nullptr;
    if (heads == 0) // (ModelKind reads 0 as "no TransformerConv model" ...)
        return fail(GNNB_ERR_INVALID, "heads 0: a TransformerConv model takes 1 .. %d heads", TF_MAX_HEADS);
    if (edge_dim == 0) // (... and as "no edge features")
        return fail(GNNB_ERR_INVALID, "edge_dim 0: a TransformerConv model with edge features takes edge_dim 1 .. %d", TFE_MAX_EDGE_DIM);
    return model_create(desc, ModelKind::transformer_edges(heads, edge_dim), host_params, num_params, out_model);
}

int gnnb_resgated_model_num_params(const gnnb_model_desc *desc) { return count_resgated_params(desc); }

int gnnb_resgated_model_create(const gnnb_model_desc *desc, const float *const *host_params, int num_params, gnnb_model **out_model)
{
    if (out_model)
        *out_model = nullptr;
    return model_create(desc, ModelKind::resgated(), host_params, num_params, out_model);
}

int gnnb_model_is_resgated(const gnnb_model *model) { return model ? model->gated : 0; }

int gnnb_resgated_edge_model_num_params(const gnnb_model_desc *desc, int edge_dim)
{
    if (edge_dim == 0) // (count_resgated_params reads 0 as "no edge features")
        return fail(GNNB_ERR_INVALID, "edge_dim 0: a ResGatedGraphConv model with edge features takes edge_dim 1 .. %d", RGE_MAX_EDGE_DIM);
    return count_resgated_params(desc, edge_dim);
}

int gnnb_resgated_edge_model_create(const gnnb_model_desc *desc, int edge_dim, const float *const *host_params, int num_params,
                                    gnnb_model **out_model)
{
    if (out_model)
        *out_model = nullptr;
    if (edge_dim == 0) // (... and as "no edge features")
        return fail(GNNB_ERR_INVALID, "edge_dim 0: a ResGatedGraphConv model with edge features takes edge_dim 1 .. %d", RGE_MAX_EDGE_DIM);
    return model_create(desc, ModelKind::resgated_edges(edge_dim), host_params, num_params, out_model);
}

int gnnb_ggnn_model_num_params(const gnnb_model_desc *desc, int steps) { return count_ggnn_params(desc, steps); }

int gnnb_ggnn_model_create(const gnnb_model_desc *desc, int steps, const float *const *host_params, int num_params, gnnb_model **out_model)
{
    if (out_model)
        *out_model = nullptr;
    if (steps == 0) // (ModelKind reads 0 as "no GatedGraphConv model")
        return fail(GNNB_ERR_INVALID, "steps 0: a GatedGraphConv model takes 1 .. %d steps per layer", GGNN_MAX_STEPS);
    return model_create(desc, ModelKind::ggnn(steps), host_params, num_params, out_model);
}

int gnnb_model_ggnn_steps(const gnnb_model *model) { return model ? model->ggnn_steps : 0; }

int gnnb_rgcn_model_num_params(const gnnb_model_desc *desc, int relations) { return count_rgcn_params(desc, relations); }

int gnnb_rgcn_model_create(const gnnb_model_desc *desc, int relations, const float *const *host_params, int num_params, gnnb_model **out_model)
{
    if (out_model)
        *out_model = nullptr;
    if (relations == 0) // (ModelKind reads 0 as "no RGCNConv model")
        return fail(GNNB_ERR_INVALID, "relations 0: an RGCNConv model takes 1 .. %d relations", RGCN_MAX_RELATIONS);
    return model_create(desc, ModelKind::rgcn(relations), host_params, num_params, out_model);
}

int gnnb_model_rgcn_relations(const gnnb_model *model) { return model ? model->rgcn_relations : 0; }

void gnnb_model_destroy(gnnb_model *model)
{
    delete model; // (~gnnb_model frees the device allocations)
}

int gnnb_model_get_desc(const gnnb_model *model, gnnb_model_desc *out_desc)
{
    if (!model || !out_desc)
        return fail(GNNB_ERR_INVALID, "null argument");
    *out_desc = model->desc;
    return GNNB_OK;
}

} // extern "C"
