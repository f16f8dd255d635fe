// Whole-graph inference entry of the UniPose image network ("whole-graph up_unipose_forward fast path"; ABI 9).
//
// The reference runs its validation / test loops as `heat = model(input)` (unipose.py:150-160); through this entry the same
// forward — ResNet-101 (resnet.py:44-124) + WASP (wasp.py:66-90) + decoder (decoder.py:38-56) with every BatchNorm folded
// into its convolution (checkpoint.fold_batchnorm) — is ONE C call on one stream: no Python, no autograd, no allocation.
// Everything below goes through the PUBLIC C ABI of this library (up_conv2d_fwd, up_maxpool3s2_fwd, up_bilinear_fwd, ...): it is at
// the same time the example of how a C / C++ application drives the kernels.  The plan owns the packed
// weight images and biases (device memory, freed by up_unipose_plan_destroy); activations live in a caller-provided workspace
// whose size up_unipose_plan_workspace() reports (tensor lifetimes are planned, buffers are reused).
//
// The launches, their order, their descriptors and their epilogues are exactly those of the drop-in module's folded inference
// forward (unipose_amd/unipose.py + modules.py after checkpoint.load_folded), so the two produce equal bits
// (tests/test_plan_*.py).  Training has no whole-graph entry: it runs through autograd.
// The image plan keeps four programs (and the three of the evaluation protocol, see ImageForm) over one weight store: the heat-maps (up_unipose_forward), the heat-maps up-sampled to the
// input size as the module does at stride != 8 (up_unipose_forward_upsampled), the joints decoded straight from the NHWC
// output of the last convolution (up_unipose_keypoints -> up_heatmap_decode; tests/test_heat_decode_*.py), and the persons of
// the box head decoded from the same NHWC output (up_unipose_persons -> up_persons_decode; tests/test_persons_*.py).
//
// The video network UniPose-LSTM (model/uniposeLSTM.py) has its entry here too (up_unipose_lstm_*, ABI 10 additions): the same
// trunk builder with the video WASP, then the centre-map hand-over, the ConvLSTM cell and the head — per frame with the caller's
// state (the module's per-frame path) or for a whole clip (its batch_frames unroll), equal bits again (tests/test_lstm_plan_*.py).
#include <algorithm>
#include <string>
#include <vector>

#include "up_common.h"

namespace up {
namespace plan {

static void* dev_alloc(size_t bytes) {
#ifdef UP_EMU
    return malloc(bytes);
#else
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
#endif
}
static void dev_free(void* p) {
    if (!p) return;
#ifdef UP_EMU
    free(p);
#else
    (void)hipFree(p);
#endif
}

static inline int rup4(int c) { return (c + 3) / 4 * 4; }

struct Tensor {
    int n, h, w, c;        // NHWC, c = physical channels
    size_t bytes;
    int first = -1, last = -1;
    size_t off = 0;
};
struct Ref {
    int id = -1;
    size_t elems = 0;      // element offset inside the tensor (row slices of the stacked WASP branches)
};
struct Conv {
    std::string name;      // state_dict prefix: <name>.weight (+ <name>.bias after folding)
    up_conv_desc d;
    int relu;
    bool has_bias;         // the folded network has a bias on every convolution but wasp.conv2
    float* w_fwd = nullptr;
    float* bias = nullptr;
    bool set = false;
};
enum Kind {
    TO_NHWC, CONV, MAXPOOL, BILINEAR, GAP, COPY, ZERO, TO_NCHW,
    DECODE,                // key points straight from the NHWC heat-maps (up_heatmap_decode), on the grid the call names
    PERSONS,               // the multi-person decode straight from the NHWC heat-maps (up_persons_decode), on their own grid
    // the evaluation protocol (ABI 10 additions): the mirrored layout pass, the flip test's combine step, final_preds from NHWC
    TO_NHWC_FLIP, MERGE, FINAL,
    // the crop in front of the network (ABI 10 addition): source frames to the trunk's input and, in `aux`, its mirror (up_crop_to_nhwc)
    CROP,
    // the video plan (ABI 10 additions): centre-map pooling, the ConvLSTM gates, and the clip layout (frame-major inside)
    POOL, LSTM0, LSTM, CLIP_TO_NHWC, CLIP_TO_NCHW, CLIP_POOL,
    // its evaluation entries (ABI 10 additions): the mirrored clip layout and pooling, decode / final_preds of frame-major maps
    // into batch-major results, the recurrent state of a stream from and to the caller's buffer
    CLIP_TO_NHWC_FLIP, CLIP_POOL_FLIP, CLIP_DECODE, CLIP_FINAL, STATE_IN, STATE_OUT
};
enum Ext { X, CENTER, PREV_HIDE, PREV_CELL, HEAT, CELL, HIDE };   // caller-owned tensors of a call
struct Op {
    Kind kind;
    Ref in, out, res, aux;
    int conv = -1;
    int n = 0;                        // images the op runs on (batch, or T * batch in the clip's trunk and head)
    Ext ext = X;                      // TO_NHWC / TO_NCHW / POOL and their clip forms: the caller's tensor
    int a = 0, b = 0, c = 0, e = 0;   // kind-specific integers (see run)
};

struct Plan {
    std::vector<Tensor> tensors;
    std::vector<Conv> convs;
    std::vector<Op> ops;
    size_t ws_bytes = 0;

    int tensor(int n, int h, int w, int c, size_t elem = 4) {
        Tensor t;
        t.n = n; t.h = h; t.w = w; t.c = c;
        t.bytes = ((size_t)n * h * w * c * elem + 255) / 256 * 256;
        tensors.push_back(t);
        return (int)tensors.size() - 1;
    }
    void touch(const Ref& r) {
        if (r.id < 0) return;
        Tensor& t = tensors[r.id];
        const int i = (int)ops.size();
        if (t.first < 0) t.first = i;
        t.last = i;
    }
    void push(Op op) {
        touch(op.in);
        touch(op.out);
        touch(op.res);
        touch(op.aux);
        ops.push_back(op);
    }
    // conv (+ folded-BatchNorm bias) (+ residual) (+ ReLU) of `images` images at (h, w) with cp physical input channels
    Ref conv(const std::string& name, Ref x, int images, int h, int w, int cp, int c, int k, int r, int stride, int pad, int dil,
             int relu, bool has_bias, Ref res = Ref(), Ref out = Ref()) {
        Conv cv;
        cv.name = name;
        cv.relu = relu;
        cv.has_bias = has_bias;
        up_conv_desc& d = cv.d;
        memset(&d, 0, sizeof(d));
        d.N = images; d.H = h; d.W = w; d.C = c; d.Cp = cp; d.ldx = cp;
        d.K = k; d.R = r; d.S = r; d.stride = stride; d.pad = pad; d.dil = dil;
        d.P = (h + 2 * pad - dil * (r - 1) - 1) / stride + 1;
        d.Q = (w + 2 * pad - dil * (r - 1) - 1) / stride + 1;
        d.Kp = rup4(k);
        d.ldy = d.Kp;
        if (out.id < 0) out.id = tensor(images, d.P, d.Q, d.ldy);
        convs.push_back(cv);
        Op op;
        op.kind = CONV;
        op.in = x; op.out = out; op.res = res;
        op.conv = (int)convs.size() - 1;
        push(op);
        return out;
    }
    void zero(Ref t) {
        Op op;
        op.kind = ZERO;
        op.out = t;
        push(op);
    }
    void copy(Ref src, int lds, Ref dst, int ldd, size_t dst_ch, long long rows, int ch) {
        Op op;
        op.kind = COPY;
        op.in = src; op.out = dst;
        op.out.elems += dst_ch;
        op.a = lds; op.b = ldd; op.c = ch; op.e = (int)rows;
        push(op);
    }
    // workspace layout: first fit over the live ranges, buffers of dead tensors are reused
    void layout() {
        struct Block {
            size_t off, bytes;
        };
        std::vector<Block> free_list;
        size_t top = 0;
        for (int i = 0; i < (int)ops.size(); ++i) {
            for (int t = 0; t < (int)tensors.size(); ++t) {
                Tensor& T = tensors[t];
                if (T.first != i) continue;
                bool placed = false;
                for (size_t f = 0; f < free_list.size(); ++f)
                    if (free_list[f].bytes >= T.bytes) {
                        T.off = free_list[f].off;
                        free_list[f].off += T.bytes;
                        free_list[f].bytes -= T.bytes;
                        placed = true;
                        break;
                    }
                if (!placed) {
                    T.off = top;
                    top += T.bytes;
                }
            }
            for (int t = 0; t < (int)tensors.size(); ++t) {
                Tensor& T = tensors[t];
                if (T.last != i) continue;
                free_list.push_back({T.off, T.bytes});
                // merge neighbours
                std::sort(free_list.begin(), free_list.end(), [](const Block& a, const Block& b) { return a.off < b.off; });
                std::vector<Block> merged;
                for (const Block& b : free_list) {
                    if (b.bytes == 0) continue;
                    if (!merged.empty() && merged.back().off + merged.back().bytes == b.off) merged.back().bytes += b.bytes;
                    else merged.push_back(b);
                }
                free_list.swap(merged);
            }
        }
        ws_bytes = top;
    }
};

// resnet.py:5-42 — conv1 / conv2 / conv3 (+ downsample) of one Bottleneck, BatchNorm folded, the residual add and the last ReLU in
// conv3's epilogue (modules.Bottleneck.forward under ops.FoldedBatchNorm)
static Ref bottleneck(Plan& p, const std::string& name, Ref x, int n, int& h, int& w, int inplanes, int planes, int stride, int dil,
                      bool down) {
    Ref y = p.conv(name + ".conv1", x, n, h, w, inplanes, inplanes, planes, 1, 1, 0, 1, 1, true);
    y = p.conv(name + ".conv2", y, n, h, w, planes, planes, planes, 3, stride, dil, dil, 1, true);
    const int ho = p.tensors[y.id].h, wo = p.tensors[y.id].w;
    Ref skip = x;
    if (down) skip = p.conv(name + ".downsample.0", x, n, h, w, inplanes, inplanes, planes * 4, 1, stride, 0, 1, 0, true);
    Ref out = p.conv(name + ".conv3", y, n, ho, wo, planes, planes, planes * 4, 1, 1, 0, 1, 1, true, skip);
    h = ho;
    w = wo;
    return out;
}

// The trunk both plans share: ResNet-101 + WASP + decoder on `n` NHWC images `x` (4 channels) of h x w, BatchNorm folded.  Returns
// decoder.last_conv.8's output (n, h/8, w/8, rup4(out_channels)) NHWC; `h` / `w` become its size.  video: the WASP of
// waspVideo.py:56-59, whose global-average-pool branch has no BatchNorm (a convolution without bias), and the heat-map tensor
// zeroed before the last convolution writes it: its spare pad channel is where the centre map goes (uniposeLSTM.py _AddCenter),
// and the ConvLSTM gate convolution reads every physical channel.
static Ref trunk(Plan& p, Ref x, int n, int& h, int& w, int output_stride, int out_channels, bool video) {
    int strides[4], dils[4];
    if (output_stride == 16) {
        const int s[4] = {1, 2, 2, 1}, d[4] = {1, 1, 1, 2};
        memcpy(strides, s, sizeof(s));
        memcpy(dils, d, sizeof(d));
    } else {
        const int s[4] = {1, 2, 1, 1}, d[4] = {1, 1, 2, 4};
        memcpy(strides, s, sizeof(s));
        memcpy(dils, d, sizeof(d));
    }
    // stem: 7x7 s2 + folded bn1 + ReLU, 3x3 s2 max-pool (resnet.py:113-117)
    x = p.conv("backbone.conv1", x, n, h, w, 4, 3, 64, 7, 2, 3, 1, 1, true);
    h = p.tensors[x.id].h;
    w = p.tensors[x.id].w;
    auto maxpool = [&](Ref in, int hh, int ww, int ch) {
        Ref out, idx;
        const int ph = (hh - 1) / 2 + 1, pw = (ww - 1) / 2 + 1;
        out.id = p.tensor(n, ph, pw, ch);
        idx.id = p.tensor(n, ph, pw, ch, 1);
        Op op;
        op.kind = MAXPOOL;
        op.in = in; op.out = out; op.res = idx;
        op.n = n;
        op.a = hh; op.b = ww; op.c = ch;
        p.push(op);
        return out;
    };
    x = maxpool(x, h, w, 64);
    h = p.tensors[x.id].h;
    w = p.tensors[x.id].w;
    // layer1..4 (resnet.py:76-111): (3, 4, 23, 3) blocks, multi-grid (1, 2, 4) in layer4
    const int planes[4] = {64, 128, 256, 512}, blocks[4] = {3, 4, 23, 3};
    int inplanes = 64;
    Ref low;
    int low_h = 0, low_w = 0;
    for (int l = 0; l < 4; ++l) {
        for (int b = 0; b < blocks[l]; ++b) {
            const int grid = l == 3 ? (b == 0 ? 1 : b == 1 ? 2 : 4) : 1;
            const bool first = b == 0;
            const bool down = first && (strides[l] != 1 || inplanes != planes[l] * 4);
            x = bottleneck(p, "backbone.layer" + std::to_string(l + 1) + "." + std::to_string(b), x, n, h, w, inplanes, planes[l],
                           first ? strides[l] : 1, grid * dils[l], down);
            inplanes = planes[l] * 4;
        }
        if (l == 0) {
            low = x;
            low_h = h;
            low_w = w;
        }
    }
    // WASP (wasp.py:66-90; modules.WASP.forward): the four branch outputs are rows of ONE (4N, h, w, 256) tensor, so that the
    // twice-applied 1x1 convolution runs as two launches over 4 N h w rows
    const int wd[4] = {output_stride == 16 ? 24 : 48, output_stride == 16 ? 18 : 36, output_stride == 16 ? 12 : 24,
                       output_stride == 16 ? 6 : 12};
    Ref stack;
    stack.id = p.tensor(4 * n, h, w, 256);
    const size_t branch = (size_t)n * h * w * 256;
    Ref b1 = stack, b2 = stack, b3 = stack, b4 = stack;
    b2.elems = branch;
    b3.elems = 2 * branch;
    b4.elems = 3 * branch;
    p.conv("wasp.aspp1.atrous_conv", x, n, h, w, 2048, 2048, 256, 1, 1, 0, wd[0], 1, true, Ref(), b1);
    p.conv("wasp.aspp2.atrous_conv", b1, n, h, w, 256, 256, 256, 3, 1, wd[1], wd[1], 1, true, Ref(), b2);
    p.conv("wasp.aspp3.atrous_conv", b2, n, h, w, 256, 256, 256, 3, 1, wd[2], wd[2], 1, true, Ref(), b3);
    p.conv("wasp.aspp4.atrous_conv", b3, n, h, w, 256, 256, 256, 3, 1, wd[3], wd[3], 1, true, Ref(), b4);
    Ref y = p.conv("wasp.conv2", stack, 4 * n, h, w, 256, 256, 256, 1, 1, 0, 1, 0, false);
    y = p.conv("wasp.conv2", y, 4 * n, h, w, 256, 256, 256, 1, 1, 0, 1, 0, false);   // the SAME weight again (wasp.py:72-80)
    // global-average-pool branch: GAP -> 1x1 (+ folded BatchNorm) + ReLU -> bilinear 1x1 -> h x w (a broadcast)
    Ref g;
    g.id = p.tensor(n, 1, 1, 2048);
    {
        Op op;
        op.kind = GAP;
        op.in = x; op.out = g;
        op.n = n;
        op.a = h * w; op.c = 2048;
        p.push(op);
    }
    g = p.conv("wasp.global_avg_pool.1", g, n, 1, 1, 2048, 2048, 256, 1, 1, 0, 1, 1, !video);
    auto bilinear = [&](Ref in, int hh, int ww, int ch, int ph, int pw) {
        Ref out;
        out.id = p.tensor(n, ph, pw, ch);
        Op op;
        op.kind = BILINEAR;
        op.in = in; op.out = out;
        op.n = n;
        op.a = hh; op.b = ww; op.c = ch; op.e = ph * 65536 + pw;
        p.push(op);
        return out;
    };
    g = bilinear(g, 1, 1, 256, h, w);
    Ref cat;
    cat.id = p.tensor(n, h, w, 1280);
    for (int i = 0; i < 4; ++i) {
        Ref s = y;
        s.elems = i * branch;
        p.copy(s, 256, cat, 1280, (size_t)i * 256, (long long)n * h * w, 256);
    }
    p.copy(g, 256, cat, 1280, 1024, (long long)n * h * w, 256);
    x = p.conv("wasp.conv1", cat, n, h, w, 1280, 1280, 256, 1, 1, 0, 1, 1, true);   // + folded bn1 + ReLU; dropout is the identity in eval
    // decoder (decoder.py:38-56)
    Ref lw = p.conv("decoder.conv1", low, n, low_h, low_w, 256, 256, 48, 1, 1, 0, 1, 1, true);
    lw = maxpool(lw, low_h, low_w, 48);
    const int dh = p.tensors[lw.id].h, dw = p.tensors[lw.id].w;
    x = bilinear(x, h, w, 256, dh, dw);
    Ref cat2;
    cat2.id = p.tensor(n, dh, dw, 320);      // 256 + 48 = 304 real channels, zero-padded to a multiple of 32
    p.zero(cat2);
    p.copy(x, 256, cat2, 320, 0, (long long)n * dh * dw, 256);
    p.copy(lw, 48, cat2, 320, 256, (long long)n * dh * dw, 48);
    x = p.conv("decoder.last_conv.0", cat2, n, dh, dw, 320, 304, 256, 3, 1, 1, 1, 1, true);
    x = p.conv("decoder.last_conv.4", x, n, dh, dw, 256, 256, 256, 3, 1, 1, 1, 1, true);
    Ref heat;
    if (video && rup4(out_channels) != out_channels) {
        heat.id = p.tensor(n, dh, dw, rup4(out_channels));
        p.zero(heat);
    }
    h = dh;
    w = dw;
    return p.conv("decoder.last_conv.8", x, n, dh, dw, 256, 256, out_channels, 1, 1, 0, 1, 0, true, Ref(), heat);
}

// One program of the image plan over one weight store (like the video plan's LstmForm below).  HEAT_MAPS: the module's forward at
// stride 8; UPSAMPLED: at stride != 8, the heat-maps bilinearly up-sampled to the input size before the layout pass
// (model/unipose.py:31-32; unipose_amd/unipose.py forward); KEYPOINTS: the trunk, then up_heatmap_decode on its NHWC output;
// PERSONS_FORM: the trunk, then up_persons_decode on its NHWC output.
// The evaluation protocol (utils/extra_utils): FLIP_HEAT: the trunk on x and on the mirrored x (up_nchw_to_nhwc_flip) over the same
// activations — every convolution launch is the one HEAT_MAPS makes — the first pass's heat-maps staying alive through the second,
// then up_flip_merge into the caller's NCHW tensor; FLIP_PREDS: the same, merged in place (NHWC), then up_final_preds; PREDS: one
// pass, then up_final_preds.  All three work on the heat-maps' own grid.
// From source frames (up_unipose_frame_heatmaps / up_unipose_frame_final_preds): FRAME_HEAT, FRAME_FLIP_HEAT, FRAME_FLIP_PREDS and
// FRAME_PREDS are HEAT_MAPS, FLIP_HEAT, FLIP_PREDS and PREDS with ONE up_crop_to_nhwc launch in place of the layout pass(es): it
// fills the trunk's input and, in the flip forms, the mirrored input too, which then stays alive through the first trunk.
enum ImageForm {
    HEAT_MAPS, UPSAMPLED, KEYPOINTS, PERSONS_FORM, FLIP_HEAT, FLIP_PREDS, PREDS,
    FRAME_HEAT, FRAME_FLIP_HEAT, FRAME_FLIP_PREDS, FRAME_PREDS, IMAGE_FORMS
};

static int build(Plan& p, const up_unipose_config& c, ImageForm form) {
    const int n = c.batch;
    int h = c.height, w = c.width;
    const bool frame = form >= FRAME_HEAT;
    if (frame) form = form == FRAME_HEAT ? HEAT_MAPS : form == FRAME_FLIP_HEAT ? FLIP_HEAT : form == FRAME_FLIP_PREDS ? FLIP_PREDS : PREDS;
    const bool flip = form == FLIP_HEAT || form == FLIP_PREDS;
    // input NCHW -> NHWC, 3 -> 4 channels (ops.ToNHWC); from frames: the crop writes NHWC itself, and the mirror beside it
    Ref x, m;
    x.id = p.tensor(n, h, w, 4);
    if (frame && flip) m.id = p.tensor(n, h, w, 4);
    {
        Op op;
        op.kind = frame ? CROP : TO_NHWC;
        op.out = x;
        op.aux = m;
        op.ext = X;
        op.n = n; op.c = 3;
        p.push(op);
    }
    x = trunk(p, x, n, h, w, c.output_stride, c.out_channels, false);
    if (flip) {
        int h2 = c.height, w2 = c.width;
        Op op;
        if (!frame) {
            m.id = p.tensor(n, h2, w2, 4);
            op.kind = TO_NHWC_FLIP;
            op.out = m;
            op.ext = X;
            op.n = n; op.c = 3;
            p.push(op);
        }
        m = trunk(p, m, n, h2, w2, c.output_stride, c.out_channels, false);
        op = Op();
        op.kind = MERGE;
        op.in = x; op.aux = m;
        if (form == FLIP_PREDS) op.out = x;      // in place: out == a with equal strides
        op.ext = HEAT;
        op.n = n; op.c = c.out_channels;
        p.push(op);
    }
    if (form == FLIP_PREDS || form == PREDS) {
        Op op;
        op.kind = FINAL;
        op.in = x;
        op.n = n; op.c = c.out_channels;
        p.push(op);
    }
    if (form == FLIP_HEAT || form == FLIP_PREDS || form == PREDS) {
        p.layout();
        return UP_OK;
    }
    if (form == KEYPOINTS || form == PERSONS_FORM) {
        Op op;
        op.kind = form == KEYPOINTS ? DECODE : PERSONS;
        op.in = x;
        op.n = n; op.c = c.out_channels;
        p.push(op);
        p.layout();
        return UP_OK;
    }
    if (form == UPSAMPLED) {
        const int ld = p.tensors[x.id].c;
        Ref up;
        up.id = p.tensor(n, c.height, c.width, ld);
        Op op;
        op.kind = BILINEAR;
        op.in = x; op.out = up;
        op.n = n;
        op.a = h; op.b = w; op.c = ld; op.e = c.height * 65536 + c.width;
        p.push(op);
        x = up;
    }
    {
        Op op;
        op.kind = TO_NCHW;
        op.in = x;
        op.ext = HEAT;
        op.n = n; op.c = c.out_channels;
        p.push(op);
    }
    p.layout();
    return UP_OK;
}

// ---- UniPose-LSTM (model/uniposeLSTM.py:67-138; the drop-in module unipose_amd/uniposeLSTM.py after checkpoint.load_folded) ----
// STEP_FIRST / STEP_NEXT: the module's per-frame path (batch_frames = False) for iter == 0 (LSTM_0) resp. iter > 0 with the caller's
// NCHW state; CLIP: its whole-clip unroll (_unroll_clip: batch_frames = batch_head = True).  The evaluation entries run the same
// launches and end differently: CLIP_KEYPOINTS decodes the NHWC output of conv5 (up_clip_heatmap_decode); CLIP_FLIP runs the whole
// clip program twice, on the clip and on the mirrored clip (up_clip_nchw_to_nhwc_flip, up_clip_avgpool9s8_flip_fwd), each pass with
// its own recurrent state, the first pass's heat-maps staying alive through the second, then up_flip_merge in place and the layout
// pass; CLIP_FLIP_PREDS: the same, then up_clip_final_preds; CLIP_PREDS: one pass, then up_clip_final_preds.  STREAM_FIRST /
// STREAM_NEXT: the step forms with the recurrent state in the caller's opaque NHWC buffer (whole padded rows copied in and out)
// and up_heatmap_decode at the end; the NCHW heat-maps are optional.
enum LstmForm { STEP_FIRST, STEP_NEXT, CLIP, CLIP_KEYPOINTS, CLIP_FLIP, CLIP_FLIP_PREDS, CLIP_PREDS, STREAM_FIRST, STREAM_NEXT, LSTM_FORMS };

struct LstmPass {
    Ref y, cells, hides;       // conv5's output and the state tensors, frame-major (T * B, h, w, .)
    int h = 0, w = 0;
};

// One pass of a video program up to conv5: the trunk once on the T * B frame-major images (T = 1 in the step and stream forms), the
// recurrence frame by frame on rows of frame-major state tensors, the head once on the T * B hidden states.  Stacked gate
// convolutions are named "lstm_0" / "lstm" (the plan builds their weights from the parts).  mirrored: the pass of the flip test.
static LstmPass lstm_pass(Plan& p, const up_unipose_lstm_config& c, LstmForm form, bool mirrored) {
    const bool clip = form >= CLIP && form <= CLIP_PREDS, next = form == STEP_NEXT || form == STREAM_NEXT;
    const int B = c.batch, T = clip ? c.frames : 1, n = T * B;
    const int hc = c.num_classes + 1, cg = c.num_classes + 2, ldo = rup4(cg);
    int h = c.height, w = c.width;
    Ref x;
    x.id = p.tensor(n, h, w, 4);
    {
        Op op;
        op.kind = !clip ? TO_NHWC : mirrored ? CLIP_TO_NHWC_FLIP : CLIP_TO_NHWC;
        op.out = x;
        op.ext = X;
        op.n = B; op.a = T; op.c = 3;
        p.push(op);
    }
    Ref heat = trunk(p, x, n, h, w, c.output_stride, hc, true);
    // _AddCenter: the pooled centre map in the heat-maps' spare pad channel; (K + 1) % 4 == 0: a hand-over tensor of rup4(K + 2)
    // channels, zeros, the heat-maps copied in
    Ref z = heat;
    if (rup4(hc) == hc) {
        z.id = p.tensor(n, h, w, ldo);
        p.zero(z);
        p.copy(heat, hc, z, ldo, 0, (long long)n * h * w, hc);
    }
    const int ldz = p.tensors[z.id].c;       // == ldo either way
    {
        Op op;
        op.kind = !clip ? POOL : mirrored ? CLIP_POOL_FLIP : CLIP_POOL;
        op.out = z;
        op.ext = CENTER;
        op.n = B; op.e = T;
        op.a = c.height; op.b = c.width; op.c = hc;
        p.push(op);
    }
    // the recurrence: cell / hide of all frames as rows of two frame-major tensors (the head reads the hidden states as one)
    Ref cells, hides;
    cells.id = p.tensor(n, h, w, ldo);
    hides.id = p.tensor(n, h, w, ldo);
    if (ldo != cg) {                         // pad channels read as zeros (the conv1 of the head reads all ldo)
        p.zero(cells);
        p.zero(hides);
    }
    const size_t frame = (size_t)B * h * w;
    for (int t = 0; t < T; ++t) {
        Ref zt = z, ct = cells, ht = hides;
        zt.elems += t * frame * ldz;
        ct.elems += t * frame * ldo;
        ht.elems += t * frame * ldo;
        Op op;
        op.n = B; op.c = cg;
        op.out = ct; op.res = ht;
        if (t == 0 && !next) {                // LSTM_0 (uniposeLSTM.py:9-24)
            op.kind = LSTM0;
            op.in = p.conv("lstm_0", zt, B, h, w, ldz, cg, 3 * cg, 3, 1, 1, 1, 0, true);
        } else {                              // LSTM (uniposeLSTM.py:27-64): ONE convolution over cat(z, prev_hide)
            Ref ph, pc;
            if (next) {
                ph.id = p.tensor(B, h, w, ldo);
                pc.id = p.tensor(B, h, w, ldo);
                Op in;
                if (form == STEP_NEXT) {      // the caller's NCHW state (unipose._state: ToNHWC, pad channels zero)
                    in.kind = TO_NHWC;
                    in.n = B; in.c = cg;
                    in.out = ph; in.ext = PREV_HIDE;
                    p.push(in);
                    in.out = pc; in.ext = PREV_CELL;
                    p.push(in);
                } else {                      // the caller's state buffer: the plan's own NHWC rows, pad channels as the plan left them
                    in.kind = STATE_IN;
                    in.out = ph; in.a = 0;
                    p.push(in);
                    in.out = pc; in.a = 1;
                    p.push(in);
                }
            } else {
                ph = hides;
                pc = cells;
                ph.elems += (t - 1) * frame * ldo;
                pc.elems += (t - 1) * frame * ldo;
            }
            Ref zh;
            zh.id = p.tensor(B, h, w, ldz + ldo);
            p.copy(zt, ldz, zh, ldz + ldo, 0, (long long)frame, ldz);
            p.copy(ph, ldo, zh, ldz + ldo, ldz, (long long)frame, ldo);
            op.kind = LSTM;
            op.in = p.conv("lstm", zh, B, h, w, ldz + ldo, ldz + ldo, 4 * cg, 3, 1, 1, 1, 0, true);
            op.aux = pc;
        }
        p.push(op);
    }
    // the head (uniposeLSTM.py:85-89, 135-138): five convolutions with bias + ReLU
    Ref y = p.conv("conv1", hides, n, h, w, ldo, cg, 128, 11, 1, 5, 1, 1, true);
    y = p.conv("conv2", y, n, h, w, 128, 128, 128, 11, 1, 5, 1, 1, true);
    y = p.conv("conv3", y, n, h, w, 128, 128, 128, 11, 1, 5, 1, 1, true);
    y = p.conv("conv4", y, n, h, w, 128, 128, 128, 1, 1, 0, 1, 1, true);
    y = p.conv("conv5", y, n, h, w, 128, 128, hc, 1, 1, 0, 1, 1, true);
    LstmPass r;
    r.y = y; r.cells = cells; r.hides = hides;
    r.h = h; r.w = w;
    return r;
}

static void build_lstm(Plan& p, const up_unipose_lstm_config& c, LstmForm form) {
    const bool clip = form >= CLIP && form <= CLIP_PREDS, stream = form == STREAM_FIRST || form == STREAM_NEXT;
    const int B = c.batch, T = clip ? c.frames : 1;
    const int hc = c.num_classes + 1, cg = c.num_classes + 2, ldo = rup4(cg);
    const LstmPass a = lstm_pass(p, c, form, false);
    Op op;
    if (form == CLIP_FLIP || form == CLIP_FLIP_PREDS) {
        const LstmPass m = lstm_pass(p, c, form, true);
        op.kind = MERGE;                       // in place (NHWC): out == a with equal strides; both passes are frame-major
        op.in = a.y; op.aux = m.y; op.out = a.y;
        op.n = T * B; op.c = hc;
        p.push(op);
    }
    if (form == CLIP_FLIP_PREDS || form == CLIP_PREDS || form == CLIP_KEYPOINTS) {
        op = Op();
        op.kind = form == CLIP_KEYPOINTS ? CLIP_DECODE : CLIP_FINAL;
        op.in = a.y;
        op.n = B; op.a = T; op.c = hc;
        p.push(op);
    }
    if (form == CLIP_FLIP_PREDS || form == CLIP_PREDS) {
        p.layout();
        return;
    }
    const size_t frame = (size_t)B * a.h * a.w;
    Ref cl = a.cells, hl = a.hides;            // the state of the last frame
    cl.elems += (T - 1) * frame * ldo;
    hl.elems += (T - 1) * frame * ldo;
    if (stream) {                              // the new state into the caller's buffer, then the joints
        op = Op();
        op.kind = STATE_OUT;
        op.in = hl; op.a = 0;
        p.push(op);
        op.in = cl; op.a = 1;
        p.push(op);
        op = Op();
        op.kind = DECODE;
        op.in = a.y;
        op.n = B; op.c = hc;
        p.push(op);
    }
    if (form != CLIP_KEYPOINTS) {
        op = Op();
        op.kind = clip ? CLIP_TO_NCHW : TO_NCHW;     // TO_NCHW is skipped where the caller passes no tensor (the stream forms' heat)
        op.in = a.y;
        op.ext = HEAT;
        op.n = B; op.a = T; op.c = hc;
        p.push(op);
    }
    if (form == CLIP_FLIP || stream) {         // a flip program has two states and returns none; a stream's state is in its buffer
        p.layout();
        return;
    }
    op = Op();
    op.kind = TO_NCHW;
    op.n = B; op.c = cg;
    op.in = cl; op.ext = CELL;
    p.push(op);
    op.in = hl; op.ext = HIDE;
    p.push(op);
    p.layout();
}

// caller-owned tensors of one call
struct Io {
    const float* x = nullptr;
    const float* center = nullptr;
    const float* prev_hide = nullptr;
    const float* prev_cell = nullptr;
    float* heat = nullptr;
    float* cell = nullptr;
    float* hide = nullptr;
    int dec_h = 0, dec_w = 0;        // DECODE: the grid, and the three outputs of up_heatmap_decode
    int32_t* idx = nullptr;
    float* preds = nullptr;
    float* maxvals = nullptr;
    int box_ch0 = 0, joint_ch0 = 0, njoints = 0, max_persons = 0;     // PERSONS: the arguments and outputs of up_persons_decode
    int32_t* count = nullptr;
    int32_t* status = nullptr;
    int32_t* kpts = nullptr;
    const int32_t* perm = nullptr;   // MERGE: the channel permutation (host); FINAL: the arguments and outputs of up_final_preds
    const double* inv = nullptr;
    int res0 = 0, res1 = 0;
    float* coords = nullptr;
    float* state = nullptr;          // STATE_IN / STATE_OUT: the caller's buffer, hide then cell, state_half elements each
    size_t state_half = 0;
    const void* src = nullptr;       // CROP: the arguments of up_crop_to_nhwc
    int src_type = 0, frames = 0, src_h = 0, src_w = 0;
    const int32_t* frame_of = nullptr;
    const int32_t* valid_hw = nullptr;
    const double* crop_inv = nullptr;
    float border = 0.f, mean = 0.f, stdv = 0.f;
    const float* in(Ext e) const { return e == X ? x : e == CENTER ? center : e == PREV_HIDE ? prev_hide : prev_cell; }
    float* out(Ext e) const { return e == HEAT ? heat : e == CELL ? cell : hide; }
};

static int run(const Plan& p, const Io& io, unsigned char* ws, void* stream, const char* what) {
    auto ptr = [&](const Ref& r) -> float* {
        return r.id < 0 ? nullptr : reinterpret_cast<float*>(ws + p.tensors[r.id].off) + r.elems;
    };
    auto T_ = [&](const Ref& r) -> const Tensor& { return p.tensors[r.id]; };
    for (const Op& op : p.ops) {
        int e = UP_OK;
        switch (op.kind) {
        case TO_NHWC:
            e = up_nchw_to_nhwc(io.in(op.ext), ptr(op.out), op.n, op.c, T_(op.out).h, T_(op.out).w, T_(op.out).c, stream);
            break;
        case CONV: {
            const Conv& cv = p.convs[op.conv];
            up_conv_epilogue ep;
            memset(&ep, 0, sizeof(ep));
            ep.bias = cv.bias;
            ep.residual = ptr(op.res);
            ep.ldr = op.res.id >= 0 ? T_(op.res).c : 0;
            ep.relu = cv.relu;
            e = up_conv2d_fwd(&cv.d, ptr(op.in), cv.w_fwd, ptr(op.out), &ep, stream);
            break;
        }
        case MAXPOOL:
            e = up_maxpool3s2_fwd(ptr(op.in), op.c, ptr(op.out), op.c, reinterpret_cast<uint8_t*>(ptr(op.res)), op.n, op.a, op.b, op.c,
                                  (op.a - 1) / 2 + 1, (op.b - 1) / 2 + 1, stream);
            break;
        case BILINEAR:
            e = up_bilinear_fwd(ptr(op.in), op.c, ptr(op.out), op.c, op.n, op.a, op.b, op.c, op.e >> 16, op.e & 65535, stream);
            break;
        case GAP:
            e = up_gap_fwd(ptr(op.in), op.c, ptr(op.out), op.n, op.a, op.c, stream);
            break;
        case COPY:
            e = up_copy2d(ptr(op.in), op.a, ptr(op.out), op.b, op.e, op.c, stream);
            break;
        case ZERO:
            if (hipMemsetAsync(ptr(op.out), 0, T_(op.out).bytes, as_stream(stream)) != hipSuccess) e = check_launch(what);
            break;
        case TO_NCHW:
            if (io.out(op.ext))
                e = up_nhwc_to_nchw(ptr(op.in), T_(op.in).c, io.out(op.ext), op.n, op.c, T_(op.in).h, T_(op.in).w, stream);
            break;
        case DECODE:
            e = up_heatmap_decode(ptr(op.in), (int64_t)T_(op.in).h * T_(op.in).w * T_(op.in).c, 1, T_(op.in).c, op.n, op.c,
                                  T_(op.in).h, T_(op.in).w, io.dec_h, io.dec_w, io.idx, io.preds, io.maxvals, stream);
            break;
        case PERSONS:
            e = up_persons_decode(ptr(op.in), (int64_t)T_(op.in).h * T_(op.in).w * T_(op.in).c, 1, T_(op.in).c, op.n, op.c, T_(op.in).h,
                                  T_(op.in).w, io.box_ch0, io.joint_ch0, io.njoints, io.max_persons, io.count, io.status, io.kpts, stream);
            break;
        case TO_NHWC_FLIP:
            e = up_nchw_to_nhwc_flip(io.in(op.ext), ptr(op.out), op.n, op.c, T_(op.out).h, T_(op.out).w, T_(op.out).c, stream);
            break;
        case CROP:
            e = up_crop_to_nhwc(io.src, io.src_type, io.frames, io.src_h, io.src_w, op.c, io.frame_of, io.valid_hw, io.crop_inv, op.n,
                                io.border, io.mean, io.stdv, ptr(op.out), ptr(op.aux), T_(op.out).h, T_(op.out).w, T_(op.out).c, stream);
            break;
        case MERGE: {
            const Tensor& t = T_(op.in);
            const int64_t sb = (int64_t)t.h * t.w * t.c;
            if (op.out.id >= 0)
                e = up_flip_merge(ptr(op.in), ptr(op.aux), sb, 1, t.c, op.n, op.c, t.h, t.w, io.perm, ptr(op.out), sb, 1, t.c, stream);
            else
                e = up_flip_merge(ptr(op.in), ptr(op.aux), sb, 1, t.c, op.n, op.c, t.h, t.w, io.perm, io.out(op.ext),
                                  (int64_t)op.c * t.h * t.w, (int64_t)t.h * t.w, 1, stream);
            break;
        }
        case FINAL:
            e = up_final_preds(ptr(op.in), (int64_t)T_(op.in).h * T_(op.in).w * T_(op.in).c, 1, T_(op.in).c, op.n, op.c, T_(op.in).h,
                               T_(op.in).w, io.res0, io.res1, io.inv, io.preds, io.coords, io.maxvals, stream);
            break;
        case POOL:
            e = up_avgpool9s8_fwd(io.center, ptr(op.out), T_(op.out).c, op.c, op.n, op.a, op.b, T_(op.out).h, T_(op.out).w, stream);
            break;
        case CLIP_POOL:
            e = up_clip_avgpool9s8_fwd(io.center, ptr(op.out), T_(op.out).c, op.c, op.n, op.e, op.a, op.b, T_(op.out).h, T_(op.out).w,
                                       stream);
            break;
        case LSTM0:
            e = up_lstm0_fwd(ptr(op.in), T_(op.in).c, ptr(op.out), ptr(op.res), T_(op.out).c, (int64_t)op.n * T_(op.in).h * T_(op.in).w,
                             op.c, stream);
            break;
        case LSTM:
            e = up_lstm_fwd(ptr(op.in), T_(op.in).c, ptr(op.aux), T_(op.aux).c, ptr(op.out), ptr(op.res), T_(op.out).c,
                            (int64_t)op.n * T_(op.in).h * T_(op.in).w, op.c, stream);
            break;
        case CLIP_TO_NHWC:
            e = up_clip_nchw_to_nhwc(io.x, ptr(op.out), op.n, op.a, op.c, T_(op.out).h, T_(op.out).w, T_(op.out).c, stream);
            break;
        case CLIP_TO_NCHW:
            e = up_clip_nhwc_to_nchw(ptr(op.in), T_(op.in).c, io.heat, op.n, op.a, op.c, T_(op.in).h, T_(op.in).w, stream);
            break;
        case CLIP_TO_NHWC_FLIP:
            e = up_clip_nchw_to_nhwc_flip(io.x, ptr(op.out), op.n, op.a, op.c, T_(op.out).h, T_(op.out).w, T_(op.out).c, stream);
            break;
        case CLIP_POOL_FLIP:
            e = up_clip_avgpool9s8_flip_fwd(io.center, ptr(op.out), T_(op.out).c, op.c, op.n, op.e, op.a, op.b, T_(op.out).h,
                                            T_(op.out).w, stream);
            break;
        case CLIP_DECODE:
            e = up_clip_heatmap_decode(ptr(op.in), (int64_t)T_(op.in).h * T_(op.in).w * T_(op.in).c, 1, T_(op.in).c, op.n, op.a, op.c,
                                       T_(op.in).h, T_(op.in).w, io.dec_h, io.dec_w, io.idx, io.preds, io.maxvals, stream);
            break;
        case CLIP_FINAL:
            e = up_clip_final_preds(ptr(op.in), (int64_t)T_(op.in).h * T_(op.in).w * T_(op.in).c, 1, T_(op.in).c, op.n, op.a, op.c,
                                    T_(op.in).h, T_(op.in).w, io.res0, io.res1, io.inv, io.preds, io.coords, io.maxvals, stream);
            break;
        case STATE_IN: {                       // whole padded rows: the pad channels stay the zeros the plan wrote
            const Tensor& t = T_(op.out);
            e = up_copy2d(io.state + op.a * io.state_half, t.c, ptr(op.out), t.c, (int64_t)t.n * t.h * t.w, t.c, stream);
            break;
        }
        case STATE_OUT: {
            const Tensor& t = T_(op.in);
            e = up_copy2d(ptr(op.in), t.c, io.state + op.a * io.state_half, t.c, (int64_t)t.n * t.h * t.w, t.c, stream);
            break;
        }
        }
        if (e) return e;
    }
    return UP_OK;
}

}  // namespace plan
}  // namespace up

using namespace up;
using up::plan::Plan;

struct up_unipose_plan {
    up_unipose_config cfg;
    Plan p;                    // HEAT_MAPS; its convolutions are the listed ones and own the weight store
    Plan up, kp, ps;           // UPSAMPLED, KEYPOINTS, PERSONS_FORM: the same trunk, so the same convolutions in the same order
    Plan fh, fp, pr;           // FLIP_HEAT, FLIP_PREDS (the trunk twice: every convolution name twice), PREDS
    Plan rh, rfh, rfp, rpr;    // FRAME_HEAT, FRAME_FLIP_HEAT, FRAME_FLIP_PREDS, FRAME_PREDS: their needs are reported per program only
    size_t ws_bytes = 0;       // the largest of the first four
    size_t flip_ws_bytes = 0;  // the largest of the next three
    Plan* prog(int form) {
        Plan* const all[up::plan::IMAGE_FORMS] = {&p, &up, &kp, &ps, &fh, &fp, &pr, &rh, &rfh, &rfp, &rpr};
        return all[form];
    }
};

extern "C" int up_unipose_plan_create(const up_unipose_config* cfg, up_unipose_plan** out) {
    UP_REQUIRE(cfg && out, UP_ERR_INVALID, "unipose_plan_create: null argument");
    UP_REQUIRE(cfg->batch > 0 && cfg->height >= 32 && cfg->width >= 32 && cfg->out_channels > 0, UP_ERR_INVALID,
               "unipose_plan_create: batch %d, input %dx%d, %d output channels", cfg->batch, cfg->height, cfg->width, cfg->out_channels);
    UP_REQUIRE(cfg->output_stride == 16 || cfg->output_stride == 8, UP_ERR_UNSUPPORTED,
               "unipose_plan_create: output stride %d (the reference builds 16 and 8, resnet.py:49-58)", cfg->output_stride);
    up_unipose_plan* pl = new (std::nothrow) up_unipose_plan();
    UP_REQUIRE(pl, UP_ERR_INVALID, "unipose_plan_create: out of host memory");
    pl->cfg = *cfg;
    for (int f = 0; f < plan::IMAGE_FORMS; ++f) {
        if (int e = up::plan::build(*pl->prog(f), pl->cfg, static_cast<plan::ImageForm>(f))) {
            delete pl;
            return e;
        }
        if (f >= plan::FRAME_HEAT) continue;
        size_t& need = f < plan::FLIP_HEAT ? pl->ws_bytes : pl->flip_ws_bytes;
        need = std::max(need, pl->prog(f)->ws_bytes);
    }
    // plan-owned device memory: one forward weight image (+ bias) per DISTINCT parameter (wasp.conv2 is applied twice)
    for (size_t i = 0; i < pl->p.convs.size(); ++i) {
        plan::Conv& cv = pl->p.convs[i];
        for (size_t j = 0; j < i; ++j)
            if (pl->p.convs[j].name == cv.name) {
                cv.w_fwd = pl->p.convs[j].w_fwd;
                cv.bias = pl->p.convs[j].bias;
            }
        if (cv.w_fwd) continue;
        const size_t nf = (size_t)cv.d.K * cv.d.R * cv.d.S * cv.d.Cp;
        cv.w_fwd = static_cast<float*>(plan::dev_alloc(nf * sizeof(float)));
        if (cv.has_bias) cv.bias = static_cast<float*>(plan::dev_alloc((size_t)cv.d.K * sizeof(float)));
        if (!cv.w_fwd || (cv.has_bias && !cv.bias)) {
            up_unipose_plan_destroy(pl);
            UP_REQUIRE(false, UP_ERR_INVALID, "unipose_plan_create: out of device memory");
        }
    }
    // the other programs share the store by NAME (the flip programs run the trunk twice)
    for (int f = 1; f < plan::IMAGE_FORMS; ++f)
        for (plan::Conv& cv : pl->prog(f)->convs)
            for (const plan::Conv& own : pl->p.convs)
                if (own.name == cv.name) {
                    cv.w_fwd = own.w_fwd;
                    cv.bias = own.bias;
                    break;
                }
    *out = pl;
    return UP_OK;
}

extern "C" void up_unipose_plan_destroy(up_unipose_plan* pl) {
    if (!pl) return;
    for (size_t i = 0; i < pl->p.convs.size(); ++i) {
        plan::Conv& cv = pl->p.convs[i];
        bool shared = false;
        for (size_t j = 0; j < i; ++j) shared = shared || pl->p.convs[j].name == cv.name;
        if (shared) continue;
        plan::dev_free(cv.w_fwd);
        plan::dev_free(cv.bias);
    }
    delete pl;
}

extern "C" int up_unipose_plan_num_convs(const up_unipose_plan* pl) { return pl ? (int)pl->p.convs.size() : UP_ERR_INVALID; }

extern "C" const char* up_unipose_plan_conv_name(const up_unipose_plan* pl, int i) {
    return (pl && i >= 0 && i < (int)pl->p.convs.size()) ? pl->p.convs[i].name.c_str() : "";
}

extern "C" int up_unipose_plan_conv_shape(const up_unipose_plan* pl, int i, int32_t* oihw, int32_t* has_bias) {
    UP_REQUIRE(pl && oihw && i >= 0 && i < (int)pl->p.convs.size(), UP_ERR_INVALID, "unipose_plan_conv_shape: bad argument");
    const plan::Conv& cv = pl->p.convs[i];
    oihw[0] = cv.d.K; oihw[1] = cv.d.C; oihw[2] = cv.d.R; oihw[3] = cv.d.S;
    if (has_bias) *has_bias = cv.has_bias ? 1 : 0;
    return UP_OK;
}

extern "C" int up_unipose_plan_set_conv(up_unipose_plan* pl, int i, const float* w_oihw, const float* bias, void* stream) {
    UP_REQUIRE(pl && w_oihw && i >= 0 && i < (int)pl->p.convs.size(), UP_ERR_INVALID, "unipose_plan_set_conv: bad argument");
    plan::Conv& cv = pl->p.convs[i];
    UP_REQUIRE((bias != nullptr) == cv.has_bias, UP_ERR_INVALID, "unipose_plan_set_conv: %s %s a bias (folded network)", cv.name.c_str(),
               cv.has_bias ? "needs" : "has no");
    if (int e = up_pack_weights(&cv.d, w_oihw, cv.w_fwd, nullptr, stream)) return e;
    if (bias)
        if (int e = up_copy2d(bias, cv.d.K, cv.bias, cv.d.K, 1, cv.d.K, stream)) return e;
    for (plan::Conv& other : pl->p.convs)
        if (other.name == cv.name) other.set = true;
    return UP_OK;
}

extern "C" size_t up_unipose_plan_workspace(const up_unipose_plan* pl) { return pl ? pl->ws_bytes : 0; }

extern "C" size_t up_unipose_plan_flip_workspace(const up_unipose_plan* pl) { return pl ? pl->flip_ws_bytes : 0; }

extern "C" size_t up_unipose_plan_program_workspace(const up_unipose_plan* pl, int program) {
    if (!pl) return 0;
    int form = program;
    if (program >= UP_PROGRAM_FROM_FRAMES) {     // the program that starts from source frames, named by the one it otherwise equals
        const int k = program - UP_PROGRAM_FROM_FRAMES;
        form = k == plan::HEAT_MAPS ? plan::FRAME_HEAT : k == plan::FLIP_HEAT ? plan::FRAME_FLIP_HEAT
               : k == plan::FLIP_PREDS ? plan::FRAME_FLIP_PREDS : k == plan::PREDS ? plan::FRAME_PREDS : -1;
    } else if (program >= plan::FRAME_HEAT) {
        form = -1;
    }
    return form >= 0 ? const_cast<up_unipose_plan*>(pl)->prog(form)->ws_bytes : 0;
}

static int image_ready(const up_unipose_plan* pl, const Plan& prog, const void* workspace, size_t ws_bytes, const char* what) {
    for (const plan::Conv& cv : pl->p.convs)
        UP_REQUIRE(cv.set, UP_ERR_INVALID, "%s: weights of %s were never set (up_unipose_plan_set_conv)", what, cv.name.c_str());
    UP_REQUIRE(ws_bytes >= prog.ws_bytes && (reinterpret_cast<uintptr_t>(workspace) & 255) == 0, UP_ERR_INVALID,
               "%s: workspace of %zu bytes (256-byte aligned) needed, got %zu", what, prog.ws_bytes, ws_bytes);
    return UP_OK;
}

extern "C" int up_unipose_forward(up_unipose_plan* pl, const float* x_nchw, float* heat_nchw, void* workspace, size_t ws_bytes,
                                  void* stream) {
    UP_REQUIRE(pl && x_nchw && heat_nchw && workspace, UP_ERR_INVALID, "unipose_forward: null argument");
    if (int e = image_ready(pl, pl->p, workspace, ws_bytes, "unipose_forward")) return e;
    plan::Io io;
    io.x = x_nchw;
    io.heat = heat_nchw;
    return plan::run(pl->p, io, static_cast<unsigned char*>(workspace), stream, "unipose_forward");
}

extern "C" int up_unipose_forward_upsampled(up_unipose_plan* pl, const float* x_nchw, float* heat_nchw, void* workspace,
                                            size_t ws_bytes, void* stream) {
    UP_REQUIRE(pl && x_nchw && heat_nchw && workspace, UP_ERR_INVALID, "unipose_forward_upsampled: null argument");
    if (int e = image_ready(pl, pl->up, workspace, ws_bytes, "unipose_forward_upsampled")) return e;
    plan::Io io;
    io.x = x_nchw;
    io.heat = heat_nchw;
    return plan::run(pl->up, io, static_cast<unsigned char*>(workspace), stream, "unipose_forward_upsampled");
}

extern "C" int up_unipose_keypoints(up_unipose_plan* pl, const float* x_nchw, int out_h, int out_w, int32_t* idx, float* preds_xy,
                                    float* maxvals, void* workspace, size_t ws_bytes, void* stream) {
    UP_REQUIRE(pl && x_nchw && preds_xy && maxvals && workspace, UP_ERR_INVALID, "unipose_keypoints: null argument");
    const plan::Tensor& heat = pl->kp.tensors[pl->kp.ops.back().in.id];
    UP_REQUIRE((out_h == heat.h && out_w == heat.w) || (out_h == pl->cfg.height && out_w == pl->cfg.width), UP_ERR_INVALID,
               "unipose_keypoints: a %d x %d grid; the plan decodes on the heat-maps' %d x %d or the input's %d x %d", out_h, out_w,
               heat.h, heat.w, pl->cfg.height, pl->cfg.width);
    if (int e = image_ready(pl, pl->kp, workspace, ws_bytes, "unipose_keypoints")) return e;
    plan::Io io;
    io.x = x_nchw;
    io.dec_h = out_h;
    io.dec_w = out_w;
    io.idx = idx;
    io.preds = preds_xy;
    io.maxvals = maxvals;
    return plan::run(pl->kp, io, static_cast<unsigned char*>(workspace), stream, "unipose_keypoints");
}

extern "C" int up_unipose_persons(up_unipose_plan* pl, const float* x_nchw, int box_ch0, int joint_ch0, int njoints, int max_persons,
                                  int32_t* count, int32_t* status, int32_t* kpts, void* workspace, size_t ws_bytes, void* stream) {
    UP_REQUIRE(pl && x_nchw && count && status && kpts && workspace, UP_ERR_INVALID, "unipose_persons: null argument");
    const int C = pl->cfg.out_channels;
    UP_REQUIRE(box_ch0 >= 0 && (int64_t)box_ch0 + 5 <= C, UP_ERR_INVALID, "unipose_persons: box channels %d..%lld, the plan has %d",
               box_ch0, (long long)box_ch0 + 4, C);
    UP_REQUIRE(joint_ch0 >= 0 && njoints >= 1 && (int64_t)joint_ch0 + njoints <= C, UP_ERR_INVALID,
               "unipose_persons: %d joint channels from %d, the plan has %d", njoints, joint_ch0, C);
    UP_REQUIRE(max_persons >= 1 && max_persons <= UP_PERSONS_CAP, UP_ERR_INVALID, "unipose_persons: max_persons %d (1..%d)", max_persons,
               UP_PERSONS_CAP);
    UP_REQUIRE((int64_t)pl->cfg.batch * max_persons * (njoints + 5) * 2 <= INT32_MAX, UP_ERR_INVALID,
               "unipose_persons: %d persons of %d rows for %d samples: an index beyond the int32 range", max_persons, njoints + 5,
               pl->cfg.batch);
    if (int e = image_ready(pl, pl->ps, workspace, ws_bytes, "unipose_persons")) return e;
    plan::Io io;
    io.x = x_nchw;
    io.box_ch0 = box_ch0;
    io.joint_ch0 = joint_ch0;
    io.njoints = njoints;
    io.max_persons = max_persons;
    io.count = count;
    io.status = status;
    io.kpts = kpts;
    return plan::run(pl->ps, io, static_cast<unsigned char*>(workspace), stream, "unipose_persons");
}

// the channel permutation of a flip-test call: refused here, before the first launch of the program
static int perm_ok(const up_unipose_plan* pl, const int32_t* perm, const char* what) {
    const int C = pl->cfg.out_channels;
    UP_REQUIRE(C <= 256, UP_ERR_UNSUPPORTED, "%s: %d output channels (up_flip_merge takes up to 256)", what, C);
    for (int j = 0; j < C; ++j)
        UP_REQUIRE(perm[j] >= 0 && perm[j] < C, UP_ERR_INVALID, "%s: perm[%d] = %d outside 0..%d", what, j, (int)perm[j], C - 1);
    return UP_OK;
}

extern "C" int up_unipose_flip_forward(up_unipose_plan* pl, const float* x_nchw, const int32_t* perm_host, float* heat_nchw,
                                       void* workspace, size_t ws_bytes, void* stream) {
    UP_REQUIRE(pl && x_nchw && perm_host && heat_nchw && workspace, UP_ERR_INVALID, "unipose_flip_forward: null argument");
    if (int e = perm_ok(pl, perm_host, "unipose_flip_forward")) return e;
    if (int e = image_ready(pl, pl->fh, workspace, ws_bytes, "unipose_flip_forward")) return e;
    plan::Io io;
    io.x = x_nchw;
    io.perm = perm_host;
    io.heat = heat_nchw;
    return plan::run(pl->fh, io, static_cast<unsigned char*>(workspace), stream, "unipose_flip_forward");
}

extern "C" int up_unipose_final_preds(up_unipose_plan* pl, const float* x_nchw, const int32_t* perm_host, const double* inv, int res0,
                                      int res1, float* preds_xy, float* coords_xy, float* maxvals, void* workspace, size_t ws_bytes,
                                      void* stream) {
    UP_REQUIRE(pl && x_nchw && preds_xy && maxvals && workspace, UP_ERR_INVALID, "unipose_final_preds: null argument");
    UP_REQUIRE(res0 > 0 && res1 > 0, UP_ERR_INVALID, "unipose_final_preds: res %d, %d", res0, res1);
    if (perm_host)
        if (int e = perm_ok(pl, perm_host, "unipose_final_preds")) return e;
    const Plan& prog = perm_host ? pl->fp : pl->pr;
    if (int e = image_ready(pl, prog, workspace, ws_bytes, "unipose_final_preds")) return e;
    plan::Io io;
    io.x = x_nchw;
    io.perm = perm_host;
    io.inv = inv;
    io.res0 = res0;
    io.res1 = res1;
    io.preds = preds_xy;
    io.coords = coords_xy;
    io.maxvals = maxvals;
    return plan::run(prog, io, static_cast<unsigned char*>(workspace), stream, "unipose_final_preds");
}

// From source frames (ABI 10 additions): the crop of up_crop_to_nhwc in front of the same programs.  Its own refusals (source type,
// sizes, frame_of == NULL with F != batch, std) come from its wrapper, which is the program's first launch: nothing runs before it.
static int frame_io(const up_unipose_plan* pl, plan::Io& io, const void* src_hwc, int src_type, int F, int Hs, int Ws,
                    const int32_t* frame_of, const int32_t* valid_hw, const double* crop_inv, float border, float mean, float stdv,
                    const char* what) {
    UP_REQUIRE(src_hwc && crop_inv, UP_ERR_INVALID, "%s: null source frames or crop maps", what);
    UP_REQUIRE(src_type == UP_PIX_U8 || src_type == UP_PIX_F32, UP_ERR_INVALID, "%s: source type %d", what, src_type);
    UP_REQUIRE(F > 0 && Hs > 0 && Ws > 0, UP_ERR_INVALID, "%s: %d frames of %d x %d", what, F, Hs, Ws);
    UP_REQUIRE(frame_of || F == pl->cfg.batch, UP_ERR_INVALID, "%s: no frame_of with %d frames for a batch of %d", what, F,
               pl->cfg.batch);
    UP_REQUIRE(stdv > 0.f, UP_ERR_INVALID, "%s: std %g", what, (double)stdv);
    io.src = src_hwc;
    io.src_type = src_type;
    io.frames = F;
    io.src_h = Hs;
    io.src_w = Ws;
    io.frame_of = frame_of;
    io.valid_hw = valid_hw;
    io.crop_inv = crop_inv;
    io.border = border;
    io.mean = mean;
    io.stdv = stdv;
    return UP_OK;
}

extern "C" int up_unipose_frame_heatmaps(up_unipose_plan* pl, const void* src_hwc, int src_type, int F, int Hs, int Ws,
                                         const int32_t* frame_of, const int32_t* valid_hw, const double* crop_inv, float border,
                                         float mean, float stdv, const int32_t* perm_host, float* heat_nchw, void* workspace,
                                         size_t ws_bytes, void* stream) {
    UP_REQUIRE(pl && heat_nchw && workspace, UP_ERR_INVALID, "unipose_frame_heatmaps: null argument");
    plan::Io io;
    if (int e = frame_io(pl, io, src_hwc, src_type, F, Hs, Ws, frame_of, valid_hw, crop_inv, border, mean, stdv, "unipose_frame_heatmaps"))
        return e;
    if (perm_host)
        if (int e = perm_ok(pl, perm_host, "unipose_frame_heatmaps")) return e;
    const Plan& prog = perm_host ? pl->rfh : pl->rh;
    if (int e = image_ready(pl, prog, workspace, ws_bytes, "unipose_frame_heatmaps")) return e;
    io.perm = perm_host;
    io.heat = heat_nchw;
    return plan::run(prog, io, static_cast<unsigned char*>(workspace), stream, "unipose_frame_heatmaps");
}

extern "C" int up_unipose_frame_final_preds(up_unipose_plan* pl, const void* src_hwc, int src_type, int F, int Hs, int Ws,
                                            const int32_t* frame_of, const int32_t* valid_hw, const double* crop_inv, float border,
                                            float mean, float stdv, const int32_t* perm_host, const double* inv, int res0, int res1,
                                            float* preds_xy, float* coords_xy, float* maxvals, void* workspace, size_t ws_bytes,
                                            void* stream) {
    UP_REQUIRE(pl && preds_xy && maxvals && workspace, UP_ERR_INVALID, "unipose_frame_final_preds: null argument");
    UP_REQUIRE(res0 > 0 && res1 > 0, UP_ERR_INVALID, "unipose_frame_final_preds: res %d, %d", res0, res1);
    plan::Io io;
    if (int e = frame_io(pl, io, src_hwc, src_type, F, Hs, Ws, frame_of, valid_hw, crop_inv, border, mean, stdv,
                         "unipose_frame_final_preds"))
        return e;
    if (perm_host)
        if (int e = perm_ok(pl, perm_host, "unipose_frame_final_preds")) return e;
    const Plan& prog = perm_host ? pl->rfp : pl->rpr;
    if (int e = image_ready(pl, prog, workspace, ws_bytes, "unipose_frame_final_preds")) return e;
    io.perm = perm_host;
    io.inv = inv;
    io.res0 = res0;
    io.res1 = res1;
    io.preds = preds_xy;
    io.coords = coords_xy;
    io.maxvals = maxvals;
    return plan::run(prog, io, static_cast<unsigned char*>(workspace), stream, "unipose_frame_final_preds");
}

// ---- UniPose-LSTM (ABI 10 additions) ------------------------------------------------------------------------------------------
// All programs (LstmForm) share one weight store: the per-frame step for the first frame (LSTM_0) and for a later one (LSTM over
// the caller's state), the whole clip, and the evaluation entries over the same launches.  Weights are stored once per distinct parameter; the ConvLSTM gate convolutions are set
// part by part under their state_dict names and stacked by the plan (modules.LSTM_0.forward / modules.LSTM.stacked): along the
// output channels, the x / h parts' input channels padded to rup4, each gate bias the fp32 sum bx + bh.
namespace up {
namespace plan {

struct Store {                 // one packed forward weight image (+ bias)
    std::string name;          // a state_dict prefix, or "lstm_0" / "lstm" for the stacked gate convolutions
    up_conv_desc d;            // descriptor of its first use (the packed image depends on K, C, Cp, R, S only)
    bool has_bias = false;
    float* w_fwd = nullptr;
    float* bias = nullptr;
    int parts = 0;             // stacked: 3 (g, i, o) or 8 (gx, ix, ox, fx, gh, ih, oh, fh), else 0
    float* stage_w = nullptr;  // stacked: the OIHW image the parts are copied into (pad channels zero)
    float* stage_b = nullptr;  // stacked: [parts][cg] the parts' biases
    bool staged = false;       // stage_w zeroed (on the stream of the first set_conv)
};
struct Entry {                 // one listed convolution
    std::string name;
    int32_t oihw[4];
    bool has_bias;
    int store;
    int part = -1;             // >= 0: slot of a stacked gate weight
    bool set = false;
};

}  // namespace plan
}  // namespace up

struct up_unipose_lstm_plan {
    up_unipose_lstm_config cfg;
    Plan prog[plan::LSTM_FORMS];
    std::vector<plan::Store> stores;
    std::vector<plan::Entry> entries;
    size_t ws_bytes = 0;       // the largest of the programs without the flip test
    size_t flip_ws_bytes = 0;  // the largest of CLIP_FLIP and CLIP_FLIP_PREDS
    size_t state_half = 0;     // elements of one (B, h, w, rup4(K + 2)) state tensor in a stream's buffer, a multiple of 64
};

extern "C" int up_unipose_lstm_plan_create(const up_unipose_lstm_config* cfg, up_unipose_lstm_plan** out) {
    UP_REQUIRE(cfg && out, UP_ERR_INVALID, "unipose_lstm_plan_create: null argument");
    UP_REQUIRE(cfg->batch > 0 && cfg->frames > 0 && cfg->height >= 32 && cfg->width >= 32 && cfg->num_classes > 0, UP_ERR_INVALID,
               "unipose_lstm_plan_create: batch %d, %d frames, input %dx%d, %d classes", cfg->batch, cfg->frames, cfg->height,
               cfg->width, cfg->num_classes);
    UP_REQUIRE(cfg->output_stride == 16 || cfg->output_stride == 8, UP_ERR_UNSUPPORTED,
               "unipose_lstm_plan_create: output stride %d (the reference builds 16 and 8, resnet.py:49-58)", cfg->output_stride);
    // the trunk's heat-maps are ceil(H / 8) high, the pooled centre map (H - 7) / 8 + 1 (AvgPool2d(9, 8, 1)): the module's
    // cat fails where they differ (H % 8 not in {0, 7}), the plan would write out of bounds
    UP_REQUIRE((cfg->height - 1) / 8 + 1 == (cfg->height - 7) / 8 + 1 && (cfg->width - 1) / 8 + 1 == (cfg->width - 7) / 8 + 1,
               UP_ERR_UNSUPPORTED,
               "unipose_lstm_plan_create: input %dx%d gives %dx%d heat-maps but %dx%d pooled centre maps (H, W %% 8 must be 0 or 7)",
               cfg->height, cfg->width, (cfg->height - 1) / 8 + 1, (cfg->width - 1) / 8 + 1, (cfg->height - 7) / 8 + 1,
               (cfg->width - 7) / 8 + 1);
    up_unipose_lstm_plan* pl = new (std::nothrow) up_unipose_lstm_plan();
    UP_REQUIRE(pl, UP_ERR_INVALID, "unipose_lstm_plan_create: out of host memory");
    pl->cfg = *cfg;
    for (int f = 0; f < plan::LSTM_FORMS; ++f) {
        plan::build_lstm(pl->prog[f], pl->cfg, static_cast<plan::LstmForm>(f));
        size_t& need = f == plan::CLIP_FLIP || f == plan::CLIP_FLIP_PREDS ? pl->flip_ws_bytes : pl->ws_bytes;
        need = std::max(need, pl->prog[f].ws_bytes);
    }
    {   // the hidden state STATE_OUT copies: its tensor's padded size
        const Plan& sp = pl->prog[plan::STREAM_FIRST];
        for (const plan::Op& op : sp.ops)
            if (op.kind == plan::STATE_OUT) pl->state_half = sp.tensors[op.in.id].bytes / sizeof(float);
    }
    // the weight store: every distinct name of the three programs
    auto store_of = [&](const std::string& name) {
        for (size_t s = 0; s < pl->stores.size(); ++s)
            if (pl->stores[s].name == name) return (int)s;
        return -1;
    };
    for (Plan& p : pl->prog)
        for (const plan::Conv& cv : p.convs) {
            if (store_of(cv.name) >= 0) continue;
            plan::Store st;
            st.name = cv.name;
            st.d = cv.d;
            st.has_bias = cv.has_bias;
            st.parts = cv.name == "lstm_0" ? 3 : cv.name == "lstm" ? 8 : 0;
            pl->stores.push_back(st);
        }
    const int cg = cfg->num_classes + 2;
    bool ok = true;
    for (plan::Store& st : pl->stores) {
        st.w_fwd = static_cast<float*>(plan::dev_alloc((size_t)st.d.K * st.d.R * st.d.S * st.d.Cp * sizeof(float)));
        if (st.has_bias) st.bias = static_cast<float*>(plan::dev_alloc((size_t)st.d.K * sizeof(float)));
        ok = ok && st.w_fwd && (!st.has_bias || st.bias);
        if (st.parts) {
            st.stage_w = static_cast<float*>(plan::dev_alloc((size_t)st.d.K * st.d.C * st.d.R * st.d.S * sizeof(float)));
            st.stage_b = static_cast<float*>(plan::dev_alloc((size_t)st.parts * cg * sizeof(float)));
            ok = ok && st.stage_w && st.stage_b;
        }
    }
    for (Plan& p : pl->prog)
        for (plan::Conv& cv : p.convs) {
            const plan::Store& st = pl->stores[store_of(cv.name)];
            cv.w_fwd = st.w_fwd;
            cv.bias = st.bias;
        }
    // the listed convolutions: the trunk in program order (wasp.conv2 twice, like the image plan), the gate parts, the head
    static const char* const gates0[3] = {"g", "i", "o"};
    static const char* const gates[8] = {"gx", "ix", "ox", "fx", "gh", "ih", "oh", "fh"};
    auto entry = [&](const std::string& name, int store, int part, int k, int c, int r, bool bias) {
        plan::Entry e;
        e.name = name;
        e.oihw[0] = k; e.oihw[1] = c; e.oihw[2] = r; e.oihw[3] = r;
        e.has_bias = bias;
        e.store = store;
        e.part = part;
        pl->entries.push_back(e);
    };
    for (const plan::Conv& cv : pl->prog[plan::STEP_FIRST].convs) {
        if (cv.name == "lstm_0") {
            for (int i = 0; i < 3; ++i)
                entry(std::string("lstm_0.conv_") + gates0[i] + "_lstm", store_of("lstm_0"), i, cg, cg, 3, true);
            for (int i = 0; i < 8; ++i)
                entry(std::string("lstm.conv_") + gates[i] + "_lstm", store_of("lstm"), i, cg, cg, 3, true);
            continue;
        }
        entry(cv.name, store_of(cv.name), -1, cv.d.K, cv.d.C, cv.d.R, cv.has_bias);
    }
    if (!ok) {
        up_unipose_lstm_plan_destroy(pl);
        UP_REQUIRE(false, UP_ERR_INVALID, "unipose_lstm_plan_create: out of device memory");
    }
    *out = pl;
    return UP_OK;
}

extern "C" void up_unipose_lstm_plan_destroy(up_unipose_lstm_plan* pl) {
    if (!pl) return;
    for (plan::Store& st : pl->stores) {
        plan::dev_free(st.w_fwd);
        plan::dev_free(st.bias);
        plan::dev_free(st.stage_w);
        plan::dev_free(st.stage_b);
    }
    delete pl;
}

extern "C" int up_unipose_lstm_plan_num_convs(const up_unipose_lstm_plan* pl) { return pl ? (int)pl->entries.size() : UP_ERR_INVALID; }

extern "C" const char* up_unipose_lstm_plan_conv_name(const up_unipose_lstm_plan* pl, int i) {
    return (pl && i >= 0 && i < (int)pl->entries.size()) ? pl->entries[i].name.c_str() : "";
}

extern "C" int up_unipose_lstm_plan_conv_shape(const up_unipose_lstm_plan* pl, int i, int32_t* oihw, int32_t* has_bias) {
    UP_REQUIRE(pl && oihw && i >= 0 && i < (int)pl->entries.size(), UP_ERR_INVALID, "unipose_lstm_plan_conv_shape: bad argument");
    const plan::Entry& e = pl->entries[i];
    memcpy(oihw, e.oihw, sizeof(e.oihw));
    if (has_bias) *has_bias = e.has_bias ? 1 : 0;
    return UP_OK;
}

extern "C" int up_unipose_lstm_plan_set_conv(up_unipose_lstm_plan* pl, int i, const float* w_oihw, const float* bias, void* stream) {
    UP_REQUIRE(pl && w_oihw && i >= 0 && i < (int)pl->entries.size(), UP_ERR_INVALID, "unipose_lstm_plan_set_conv: bad argument");
    plan::Entry& en = pl->entries[i];
    plan::Store& st = pl->stores[en.store];
    UP_REQUIRE((bias != nullptr) == en.has_bias, UP_ERR_INVALID, "unipose_lstm_plan_set_conv: %s %s a bias (folded network)",
               en.name.c_str(), en.has_bias ? "needs" : "has no");
    if (en.part < 0) {
        if (int e = up_pack_weights(&st.d, w_oihw, st.w_fwd, nullptr, stream)) return e;
        if (bias)
            if (int e = up_copy2d(bias, st.d.K, st.bias, st.d.K, 1, st.d.K, stream)) return e;
        for (plan::Entry& other : pl->entries)
            if (other.name == en.name) other.set = true;
        return UP_OK;
    }
    // a gate part: rows [gate * cg, (gate + 1) * cg) of the stacked OIHW image, input channels from xoff on
    const int cg = pl->cfg.num_classes + 2, taps = st.d.R * st.d.S;
    const int gate = en.part % 4, xoff = st.parts == 8 && en.part >= 4 ? st.d.C / 2 : 0;
    if (!st.staged) {
        if (hipMemsetAsync(st.stage_w, 0, (size_t)st.d.K * st.d.C * taps * sizeof(float), as_stream(stream)) != hipSuccess)
            return check_launch("unipose_lstm_plan_set_conv memset");
        st.staged = true;
    }
    if (int e = up_copy2d(w_oihw, cg * taps, st.stage_w + ((size_t)gate * cg * st.d.C + xoff) * taps, st.d.C * taps, cg, cg * taps,
                          stream))
        return e;
    if (int e = up_copy2d(bias, cg, st.stage_b + (size_t)en.part * cg, cg, 1, cg, stream)) return e;
    en.set = true;
    for (const plan::Entry& other : pl->entries)
        if (other.store == en.store && !other.set) return UP_OK;
    // every part is set: the stacked bias (LSTM_0: g | i | o; LSTM: bx + bh per gate) and the packed image
    int e = st.parts == 3 ? up_copy2d(st.stage_b, 3 * cg, st.bias, 3 * cg, 1, 3 * cg, stream)
                          : up_add2d(st.stage_b, cg, st.stage_b + 4 * cg, cg, st.bias, cg, 4, cg, stream);
    if (e) return e;
    return up_pack_weights(&st.d, st.stage_w, st.w_fwd, nullptr, stream);
}

extern "C" size_t up_unipose_lstm_plan_workspace(const up_unipose_lstm_plan* pl) { return pl ? pl->ws_bytes : 0; }

extern "C" size_t up_unipose_lstm_plan_flip_workspace(const up_unipose_lstm_plan* pl) { return pl ? pl->flip_ws_bytes : 0; }

extern "C" size_t up_unipose_lstm_plan_program_workspace(const up_unipose_lstm_plan* pl, int program) {
    return pl && program >= 0 && program < plan::LSTM_FORMS ? pl->prog[program].ws_bytes : 0;
}

extern "C" size_t up_unipose_lstm_plan_state_bytes(const up_unipose_lstm_plan* pl) {
    return pl ? 2 * pl->state_half * sizeof(float) : 0;
}

// `need`: up_unipose_lstm_plan_workspace() for step and clip (as ever), the program's own for the evaluation entries
static int lstm_ready(const up_unipose_lstm_plan* pl, size_t need, const void* workspace, size_t ws_bytes, const char* what) {
    for (const plan::Entry& e : pl->entries)
        UP_REQUIRE(e.set, UP_ERR_INVALID, "%s: weights of %s were never set (up_unipose_lstm_plan_set_conv)", what, e.name.c_str());
    UP_REQUIRE(ws_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 255) == 0, UP_ERR_WORKSPACE,
               "%s: workspace of %zu bytes (256-byte aligned) needed, got %zu", what, need, ws_bytes);
    return UP_OK;
}

extern "C" int up_unipose_lstm_step(up_unipose_lstm_plan* pl, const float* x_nchw, const float* center_nchw, const float* prev_hide,
                                    const float* prev_cell, float* heat_nchw, float* cell_nchw, float* hide_nchw, void* workspace,
                                    size_t ws_bytes, void* stream) {
    UP_REQUIRE(pl && x_nchw && center_nchw && heat_nchw && cell_nchw && hide_nchw && workspace, UP_ERR_INVALID,
               "unipose_lstm_step: null argument");
    UP_REQUIRE((prev_hide == nullptr) == (prev_cell == nullptr), UP_ERR_INVALID,
               "unipose_lstm_step: prev_hide and prev_cell are both given (a later frame) or both NULL (the first frame)");
    if (int e = lstm_ready(pl, pl->ws_bytes, workspace, ws_bytes, "unipose_lstm_step")) return e;
    plan::Io io;
    io.x = x_nchw;
    io.center = center_nchw;
    io.prev_hide = prev_hide;
    io.prev_cell = prev_cell;
    io.heat = heat_nchw;
    io.cell = cell_nchw;
    io.hide = hide_nchw;
    return plan::run(pl->prog[prev_hide ? plan::STEP_NEXT : plan::STEP_FIRST], io, static_cast<unsigned char*>(workspace), stream,
                     "unipose_lstm_step");
}

extern "C" int up_unipose_lstm_clip(up_unipose_lstm_plan* pl, const float* x, const float* center, float* heat, float* cell_last,
                                    float* hide_last, void* workspace, size_t ws_bytes, void* stream) {
    UP_REQUIRE(pl && x && center && heat && workspace, UP_ERR_INVALID, "unipose_lstm_clip: null argument");
    if (int e = lstm_ready(pl, pl->ws_bytes, workspace, ws_bytes, "unipose_lstm_clip")) return e;
    plan::Io io;
    io.x = x;
    io.center = center;
    io.heat = heat;
    io.cell = cell_last;
    io.hide = hide_last;
    return plan::run(pl->prog[plan::CLIP], io, static_cast<unsigned char*>(workspace), stream, "unipose_lstm_clip");
}

// ---- the evaluation entries of the video plan (ABI 10 additions) ---------------------------------------------------------------
extern "C" int up_unipose_lstm_clip_keypoints(up_unipose_lstm_plan* pl, const float* x, const float* center, int out_h, int out_w,
                                              int32_t* idx, float* preds_xy, float* maxvals, float* cell_last, float* hide_last,
                                              void* workspace, size_t ws_bytes, void* stream) {
    UP_REQUIRE(pl && x && center && preds_xy && maxvals && workspace, UP_ERR_INVALID, "unipose_lstm_clip_keypoints: null argument");
    const int h = (pl->cfg.height - 1) / 8 + 1, w = (pl->cfg.width - 1) / 8 + 1;
    UP_REQUIRE((out_h == h && out_w == w) || (out_h == pl->cfg.height && out_w == pl->cfg.width), UP_ERR_INVALID,
               "unipose_lstm_clip_keypoints: a %d x %d grid; the plan decodes on the heat-maps' %d x %d or the input's %d x %d", out_h,
               out_w, h, w, pl->cfg.height, pl->cfg.width);
    const Plan& prog = pl->prog[plan::CLIP_KEYPOINTS];
    if (int e = lstm_ready(pl, prog.ws_bytes, workspace, ws_bytes, "unipose_lstm_clip_keypoints")) return e;
    plan::Io io;
    io.x = x;
    io.center = center;
    io.dec_h = out_h;
    io.dec_w = out_w;
    io.idx = idx;
    io.preds = preds_xy;
    io.maxvals = maxvals;
    io.cell = cell_last;
    io.hide = hide_last;
    return plan::run(prog, io, static_cast<unsigned char*>(workspace), stream, "unipose_lstm_clip_keypoints");
}

// the channel permutation of a flip-test call: refused here, before the first launch of the program (like perm_ok)
static int lstm_perm_ok(const up_unipose_lstm_plan* pl, const int32_t* perm, const char* what) {
    const int C = pl->cfg.num_classes + 1;
    UP_REQUIRE(C <= 256, UP_ERR_UNSUPPORTED, "%s: %d heat-map channels (up_flip_merge takes up to 256)", what, C);
    for (int j = 0; j < C; ++j)
        UP_REQUIRE(perm[j] >= 0 && perm[j] < C, UP_ERR_INVALID, "%s: perm[%d] = %d outside 0..%d", what, j, (int)perm[j], C - 1);
    return UP_OK;
}

extern "C" int up_unipose_lstm_clip_flip(up_unipose_lstm_plan* pl, const float* x, const float* center, const int32_t* perm_host,
                                         float* heat, void* workspace, size_t ws_bytes, void* stream) {
    UP_REQUIRE(pl && x && center && perm_host && heat && workspace, UP_ERR_INVALID, "unipose_lstm_clip_flip: null argument");
    if (int e = lstm_perm_ok(pl, perm_host, "unipose_lstm_clip_flip")) return e;
    const Plan& prog = pl->prog[plan::CLIP_FLIP];
    if (int e = lstm_ready(pl, prog.ws_bytes, workspace, ws_bytes, "unipose_lstm_clip_flip")) return e;
    plan::Io io;
    io.x = x;
    io.center = center;
    io.perm = perm_host;
    io.heat = heat;
    return plan::run(prog, io, static_cast<unsigned char*>(workspace), stream, "unipose_lstm_clip_flip");
}

extern "C" int up_unipose_lstm_clip_final_preds(up_unipose_lstm_plan* pl, const float* x, const float* center, const int32_t* perm_host,
                                                const double* inv, int res0, int res1, float* preds_xy, float* coords_xy,
                                                float* maxvals, void* workspace, size_t ws_bytes, void* stream) {
    UP_REQUIRE(pl && x && center && preds_xy && maxvals && workspace, UP_ERR_INVALID, "unipose_lstm_clip_final_preds: null argument");
    UP_REQUIRE(res0 > 0 && res1 > 0, UP_ERR_INVALID, "unipose_lstm_clip_final_preds: res %d, %d", res0, res1);
    if (perm_host)
        if (int e = lstm_perm_ok(pl, perm_host, "unipose_lstm_clip_final_preds")) return e;
    const Plan& prog = pl->prog[perm_host ? plan::CLIP_FLIP_PREDS : plan::CLIP_PREDS];
    if (int e = lstm_ready(pl, prog.ws_bytes, workspace, ws_bytes, "unipose_lstm_clip_final_preds")) return e;
    plan::Io io;
    io.x = x;
    io.center = center;
    io.perm = perm_host;
    io.inv = inv;
    io.res0 = res0;
    io.res1 = res1;
    io.preds = preds_xy;
    io.coords = coords_xy;
    io.maxvals = maxvals;
    return plan::run(prog, io, static_cast<unsigned char*>(workspace), stream, "unipose_lstm_clip_final_preds");
}

extern "C" int up_unipose_lstm_stream_keypoints(up_unipose_lstm_plan* pl, const float* x_nchw, const float* center_nchw, void* state,
                                                int first, int out_h, int out_w, int32_t* idx, float* preds_xy, float* maxvals,
                                                float* heat_nchw, void* workspace, size_t ws_bytes, void* stream) {
    UP_REQUIRE(pl && x_nchw && center_nchw && preds_xy && maxvals && workspace, UP_ERR_INVALID,
               "unipose_lstm_stream_keypoints: null argument");
    UP_REQUIRE(state && (reinterpret_cast<uintptr_t>(state) & 255) == 0, UP_ERR_INVALID,
               "unipose_lstm_stream_keypoints: a 256-byte aligned state buffer of up_unipose_lstm_plan_state_bytes() bytes is needed");
    const int h = (pl->cfg.height - 1) / 8 + 1, w = (pl->cfg.width - 1) / 8 + 1;
    UP_REQUIRE((out_h == h && out_w == w) || (out_h == pl->cfg.height && out_w == pl->cfg.width), UP_ERR_INVALID,
               "unipose_lstm_stream_keypoints: a %d x %d grid; the plan decodes on the heat-maps' %d x %d or the input's %d x %d", out_h,
               out_w, h, w, pl->cfg.height, pl->cfg.width);
    const Plan& prog = pl->prog[first ? plan::STREAM_FIRST : plan::STREAM_NEXT];
    if (int e = lstm_ready(pl, prog.ws_bytes, workspace, ws_bytes, "unipose_lstm_stream_keypoints")) return e;
    plan::Io io;
    io.x = x_nchw;
    io.center = center_nchw;
    io.state = static_cast<float*>(state);
    io.state_half = pl->state_half;
    io.dec_h = out_h;
    io.dec_w = out_w;
    io.idx = idx;
    io.preds = preds_xy;
    io.maxvals = maxvals;
    io.heat = heat_nchw;
    return plan::run(prog, io, static_cast<unsigned char*>(workspace), stream, "unipose_lstm_stream_keypoints");
}
