// Whole-graph inference entries of the two networks ("whole-graph up_unipose_forward fast path"; ABI 10).
//
// The reference runs its validation / test loops as `heat = model(input)` (unipose.py:150-160); through these entries the same
// forward — ResNet-101 (resnet.py:44-124) + WASP (wasp.py:66-90) + decoder (decoder.py:38-56) with every BatchNorm folded
// into its convolution (checkpoint.fold_batchnorm) — is ONE C call on one stream: no Python, no autograd, no allocation.
// Everything below goes through the PUBLIC C ABI of this library (up_conv2d_fwd, up_maxpool3s2_fwd, up_bilinear_fwd, ...): it is at
// the same time the example of how a C / C++ application drives the kernels.  A plan owns the packed
// weight images and biases (device memory, freed by its destroy); activations live in a caller-provided workspace whose size
// the plan reports (tensor lifetimes are planned, buffers are reused).
//
// The launches, their order, their descriptors and their epilogues are exactly those of the drop-in modules' folded inference
// forwards (unipose_amd/unipose.py, uniposeLSTM.py + modules.py after checkpoint.load_folded), so the two produce equal bits
// (tests/test_plan_*.py, tests/test_lstm_plan_*.py).  Training has no whole-graph entry: it runs through autograd.
// The image plan also runs in bf16 STORAGE (up_unipose_plan_create_t with UP_DT_BF16): the same programs with bf16 tensors and
// weight images behind the fp32 stem, the launches of the folded module under ops.set_conv_math("bf16s") — equal bits again
// (tests/test_plan_bf16_*.py).  The element type is a parameter of trunk() and of the weight store.  The video plan takes it too
// (up_unipose_lstm_plan_create_t): a bf16 trunk that hands over fp32 heat-maps, the ConvLSTM state and the head fp32 tensors whose
// convolutions of 32-aligned input width run on bf16 operands, as the module's do (tests/test_lstm_plan_bf16_*.py).
//
// What the file holds, top to bottom:
//   Plan        one program: tensors, convolutions, ops, and the first-fit workspace layout over the tensors' live ranges
//   trunk       the builder both networks share
//   Program     what a program is made of (input, passes, ending, recurrent state), its public number and the workspace figure it
//               counts toward; IMAGE_PROGRAMS and LSTM_PROGRAMS are the two tables, build() and build_lstm() read one row each
//   run         the launches of one program, with the caller's tensors of the call in an Io
//   Weights     one store per distinct parameter and the list of convolutions the caller sets, for both plans
//   launch      "weights set, workspace large enough, then run", and the argument checks both plans make
//   up_unipose_*, up_unipose_lstm_*    the C entries: each checks its own required pointers, fills its Io and launches one program
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
static inline int rup32(int c) { return (c + 31) / 32 * 32; }

struct Tensor {
    int n, h, w, c;        // NHWC, c = physical channels
    size_t elem;           // bytes per element: 4 fp32, 2 bf16 (bf16 storage), 1 the max-pool's index tensor
    size_t bytes;
    int first = -1, last = -1;
    size_t off = 0;
};
struct Ref {
    int id = -1;
    size_t elems = 0;      // offset inside the tensor in ITS elements (row slices of the stacked WASP branches)
};
struct Conv {
    std::string name;      // state_dict prefix: <name>.weight (+ <name>.bias after folding)
    up_conv_desc d;
    int relu;
    bool has_bias;         // the folded network has a bias on every convolution but wasp.conv2
    int math = UP_MATH_F32;   // UP_MATH_F32: up_conv2d_fwd; UP_MATH_BF16S / UP_MATH_BF16S_F32OUT: up_conv2d_fwd_bf16 on bf16 tensors;
                              // UP_MATH_BF16: up_conv2d_fwd_bf16 on fp32 tensors (bf16 operands: the weight's hi plane)
    float* w_fwd = nullptr;   // the plan's store of that name (Weights::bind): the fp32 image, or the bf16 hi plane
    float* bias = nullptr;
};
// one Kind per C function called (STATE_IN / STATE_OUT: up_copy2d from / to the caller's state buffer; GATHER / SERVE:
// up_lstm_state_gather / up_lstm_serve_fwd on the caller's state pool)
enum Kind {
    TO_NHWC, CONV, MAXPOOL, BILINEAR, GAP, COPY, ZERO, TO_NCHW, DECODE, PERSONS, TO_NHWC_FLIP, MERGE, FINAL, CROP,
    POOL, LSTM0, LSTM, CLIP_TO_NHWC, CLIP_TO_NCHW, CLIP_POOL, CLIP_TO_NHWC_FLIP, CLIP_POOL_FLIP, CLIP_DECODE, CLIP_FINAL,
    STATE_IN, STATE_OUT, CLIP_CROP, CENTER_POOL, CLIP_CENTER_POOL, CLIP_CENTER_POOL_FLIP, CLIP_MERGE, GATHER, SERVE
};
enum When { ALWAYS, ANY_FIRST, ANY_NEXT };   // a serving call: launched whatever its table says, or only where a sample is first or
                                             // idle, or only where one continues
enum Ext { X, CENTER, PREV_HIDE, PREV_CELL, HEAT, CELL, HIDE };   // caller-owned tensors of a call
// Sizes, strides and physical channel counts come from the tensors an op names; the fields below are what they do not hold.
struct Op {
    Kind kind;
    Ref in, out, res, aux;
    int conv = -1;             // CONV: index into the program's convolutions
    Ext ext = X;               // the layout passes and MERGE: the caller's tensor
    int n = 0;                 // images the launch works on: the batch B, or T * B in the clip's trunk and head
    int frames = 1;            // the clip kinds: T
    int fi = 0;                // the clip kinds that write frame-major images, in a one-pass flip row: images per frame (2 B) of the
                               // tensor written, through the kernel's _strided entry; 0: the plain entry
    int ch = 0;                // logical channels the launch reads or writes (<= the tensors' physical ones)
    int coff = 0;              // the pooling kinds: the channel of `out` the pooled centre map goes to
    int src_h = 0, src_w = 0;  // the pooling kinds: size of the caller's centre maps
    int lds = 0, ldd = 0;      // COPY: row strides of source and destination, in elements
    int64_t rows = 0;          // COPY: rows of `ch` elements
    int half = 0;              // STATE_IN / STATE_OUT: 0 the hidden state, 1 the cell state of the caller's buffer
    When when = ALWAYS;        // the serving programs: skipped at run time where no sample of the call needs it
};

struct Plan {
    std::vector<Tensor> tensors;
    std::vector<Conv> convs;
    std::vector<Op> ops;
    size_t ws_bytes = 0;
    // layout(): let the free block under the top grow into a tensor that fits nowhere.  The bf16 image plan sets it: its largest
    // tensor is the up-sampled fp32 maps at the end of program 1 (rup32 lanes), larger than anything the bf16 trunk leaves free.
    // The bf16 video plan sets it too: behind the fp32 stem the bf16 tensors leave free blocks a later, larger tensor can grow from.
    // The fp32 plans keep the layout, and so the workspace figures, they always had.
    bool grow_tail = false;
    int dt = UP_DT_F32;        // the plan's storage: what conv() picks the arithmetic of an fp32 tensor's convolution by

    int tensor(int n, int h, int w, int c, size_t elem = 4) {
        Tensor t;
        t.n = n; t.h = h; t.w = w; t.c = c;
        t.elem = elem;
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
    // conv (+ folded-BatchNorm bias) (+ residual) (+ ReLU) of `images` images at (h, w) with cp physical input channels.  The
    // kernels follow the tensor's type (ops.conv_fwd_raw): a bf16 input runs up_conv2d_fwd_bf16 in bf16 storage and the output is
    // padded to a multiple of 32 channels (ops.make_desc); f32out: the network's last convolution, bf16 in, fp32 out.  A padded
    // output the plan makes itself is zeroed first, as the module allocates it: the launch writes lanes [0, K) only.  An fp32
    // tensor in a bf16 plan with cp % 32 == 0 runs up_conv2d_fwd_bf16 too, with UP_MATH_BF16: fp32 in and out (rup4 lanes), the
    // operands rounded to bf16, the weight's hi plane only; any other fp32 tensor up_conv2d_fwd.
    Ref conv(const std::string& name, Ref x, int images, int h, int w, int cp, int c, int k, int r, int stride, int pad, int dil,
             int relu, bool has_bias, Ref res = Ref(), Ref out = Ref(), bool f32out = false) {
        const bool b16 = tensors[x.id].elem == 2;
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
        d.Kp = b16 ? rup32(k) : rup4(k);
        d.ldy = d.Kp;
        if (b16) cv.math = f32out ? UP_MATH_BF16S_F32OUT : UP_MATH_BF16S;
        else cv.math = dt == UP_DT_BF16 && cp % 32 == 0 ? UP_MATH_BF16 : UP_MATH_F32;
        if (out.id < 0) {
            out.id = tensor(images, d.P, d.Q, d.ldy, b16 && !f32out ? 2 : 4);
            if (b16 && d.ldy != k) zero(out);
        }
        convs.push_back(cv);
        Op op;
        op.kind = CONV;
        op.in = x; op.out = out; op.res = res;
        op.conv = (int)convs.size() - 1;
        push(op);
        return out;
    }
    // an op from a tensor into a new one of out_h x out_w and as many channels: the two poolings and the bilinear resize
    // (out_elem: the element size of the result where it is not the input's)
    Ref resample(Kind kind, Ref in, int out_h, int out_w, size_t res_elem = 0, size_t out_elem = 0) {
        const Tensor t = tensors[in.id];
        Op op;
        op.kind = kind;
        op.in = in;
        op.out.id = tensor(t.n, out_h, out_w, t.c, out_elem ? out_elem : t.elem);
        if (res_elem) op.res.id = tensor(t.n, out_h, out_w, t.c, res_elem);
        op.n = t.n;
        push(op);
        return op.out;
    }
    Ref maxpool(Ref in, size_t out_elem = 0) {      // 3x3 stride 2 with its uint8 index tensor
        return resample(MAXPOOL, in, (tensors[in.id].h - 1) / 2 + 1, (tensors[in.id].w - 1) / 2 + 1, 1, out_elem);
    }
    void zero(Ref t) {
        Op op;
        op.kind = ZERO;
        op.out = t;
        push(op);
    }
    void copy(Ref src, int lds, Ref dst, int ldd, size_t dst_ch, int64_t rows, int ch) {
        Op op;
        op.kind = COPY;
        op.in = src; op.out = dst;
        op.out.elems += dst_ch;
        op.lds = lds; op.ldd = ldd; op.rows = rows; op.ch = ch;
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
                if (!placed) {       // no free block holds it: at the top; grow_tail: from the start of a free block that ends there
                    T.off = top;
                    for (Block& b : free_list)
                        if (grow_tail && b.bytes && b.off + b.bytes == top) {
                            T.off = b.off;
                            b.bytes = 0;
                        }
                    top = T.off + T.bytes;
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
// dt: the storage behind the stem (UP_DT_F32 / UP_DT_BF16).  In bf16 storage the launches are those of the folded module under
// ops.set_conv_math("bf16s"): the stem stays fp32 (4 input channels: no multiple of 32), its max-pool writes bf16
// (modules.ResNet.forward), every tensor behind it is bf16 with convolution outputs padded to 32 channels, and the last
// convolution writes fp32 maps of rup32(out_channels) channels (modules.Decoder.forward, out_f32): a tensor of its own, zeroed, in
// the video plan too, whose hand-over tensor lstm_pass() then makes.
static Ref trunk(Plan& p, Ref x, int n, int& h, int& w, int output_stride, int out_channels, bool video, int dt) {
    const size_t elem = dt == UP_DT_BF16 ? 2 : 4;
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
    x = p.maxpool(x, elem);
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
    stack.id = p.tensor(4 * n, h, w, 256, elem);
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
    Ref g = p.resample(GAP, x, 1, 1);
    g = p.conv("wasp.global_avg_pool.1", g, n, 1, 1, 2048, 2048, 256, 1, 1, 0, 1, 1, !video);
    g = p.resample(BILINEAR, g, h, w);
    Ref cat;
    cat.id = p.tensor(n, h, w, 1280, elem);
    for (int i = 0; i < 4; ++i) {
        Ref s = y;
        s.elems = i * branch;
        p.copy(s, 256, cat, 1280, (size_t)i * 256, (int64_t)n * h * w, 256);
    }
    p.copy(g, 256, cat, 1280, 1024, (int64_t)n * h * w, 256);
    x = p.conv("wasp.conv1", cat, n, h, w, 1280, 1280, 256, 1, 1, 0, 1, 1, true);   // + folded bn1 + ReLU; dropout is the identity in eval
    // decoder (decoder.py:38-56)
    Ref lw = p.conv("decoder.conv1", low, n, low_h, low_w, 256, 256, 48, 1, 1, 0, 1, 1, true);
    lw = p.maxpool(lw);
    const int dh = p.tensors[lw.id].h, dw = p.tensors[lw.id].w;
    x = p.resample(BILINEAR, x, dh, dw);
    Ref cat2;
    cat2.id = p.tensor(n, dh, dw, 320, elem);      // 256 + 48 = 304 real channels, zero-padded to a multiple of 32
    const int lc = p.tensors[lw.id].c;       // 48; in bf16 storage 64 physical channels, the pad lanes zeros: they fill cat2
    if (256 + lc < 320) p.zero(cat2);
    p.copy(x, 256, cat2, 320, 0, (int64_t)n * dh * dw, 256);
    p.copy(lw, lc, cat2, 320, 256, (int64_t)n * dh * dw, lc);
    x = p.conv("decoder.last_conv.0", cat2, n, dh, dw, 320, 304, 256, 3, 1, 1, 1, 1, true);
    x = p.conv("decoder.last_conv.4", x, n, dh, dw, 256, 256, 256, 3, 1, 1, 1, 1, true);
    Ref heat;
    if (video && dt != UP_DT_BF16 && rup4(out_channels) != out_channels) {
        heat.id = p.tensor(n, dh, dw, rup4(out_channels));
        p.zero(heat);
    }
    h = dh;
    w = dw;
    return p.conv("decoder.last_conv.8", x, n, dh, dw, 256, 256, out_channels, 1, 1, 0, 1, 0, true, Ref(), heat, dt == UP_DT_BF16);
}

// ---- what a program is made of ---------------------------------------------------------------------------------------------------
// the caller's NCHW batch; source frames through up_crop_to_nhwc; a (B, T, ...) clip; a clip of source frames through
// up_clip_crop_to_nhwc
enum Input { IN_NCHW, IN_FRAMES, IN_CLIP, IN_CLIP_FRAMES };
enum Ending {
    END_HEAT,          // NCHW heat-maps on their own grid
    END_UPSAMPLED,     // ... bilinearly up-sampled to the input size first, as the module does at stride != 8 (model/unipose.py:31-32)
    END_DECODE,        // key points straight from the NHWC maps (up_heatmap_decode), on the grid the call names
    END_PERSONS,       // the multi-person decode straight from the NHWC maps (up_persons_decode), on their own grid
    END_FINAL          // up_final_preds straight from the NHWC maps
};
enum Counts { COUNTS_OWN, COUNTS_PLAIN, COUNTS_FLIP };    // toward neither figure, workspace() or flip_workspace()
// the recurrent state: none, the caller's NCHW tensors, its opaque NHWC buffer, its pool of per-stream records
enum State { STATE_NONE, STATE_NCHW, STATE_BUFFER, STATE_POOL };
struct Program {
    int number;        // as up_*_plan_program_workspace() takes it
    Input input;
    bool flip;         // the flip test: the network on the input and on its mirror over the same activations, then up_flip_merge;
                       // in a plan created with UP_PLAN_FLIP_ONE_PASS these rows run ONE pass over 2 B images instead
    Ending end;
    Counts counts;
    State from = STATE_NONE, to = STATE_NONE;     // the video plan: where the state of the frame before comes from (none: LSTM_0)
                                                  // and where the new one goes
};

// The image plan.  Every convolution launch of a flip program is one the plain program makes, the first pass's heat-maps staying alive
// through the second.  From frames ONE up_crop_to_nhwc launch stands in place of the layout pass(es): it fills the trunk's input
// and, in the flip programs, the mirrored input too, which then stays alive through the first trunk — so those need more than
// flip_workspace() and report their need per program only.  All but UPSAMPLED and DECODE work on the heat-maps' own grid.
// With UP_PLAN_FLIP_ONE_PASS the rows with flip == true are built by build_one_pass() (their need: a forward at batch 2 B, with or
// without frames); every other row is built as ever.
static const Program IMAGE_PROGRAMS[] = {
    {0, IN_NCHW, false, END_HEAT, COUNTS_PLAIN},        // up_unipose_forward; its convolutions are the listed ones
    {1, IN_NCHW, false, END_UPSAMPLED, COUNTS_PLAIN},   // up_unipose_forward_upsampled
    {2, IN_NCHW, false, END_DECODE, COUNTS_PLAIN},      // up_unipose_keypoints
    {3, IN_NCHW, false, END_PERSONS, COUNTS_PLAIN},     // up_unipose_persons
    {4, IN_NCHW, true, END_HEAT, COUNTS_FLIP},          // up_unipose_flip_forward
    {5, IN_NCHW, true, END_FINAL, COUNTS_FLIP},         // up_unipose_final_preds with ...
    {6, IN_NCHW, false, END_FINAL, COUNTS_FLIP},        // ... and without the flip test
    {UP_PROGRAM_FROM_FRAMES + 0, IN_FRAMES, false, END_HEAT, COUNTS_OWN},     // up_unipose_frame_heatmaps
    {UP_PROGRAM_FROM_FRAMES + 4, IN_FRAMES, true, END_HEAT, COUNTS_OWN},
    {UP_PROGRAM_FROM_FRAMES + 5, IN_FRAMES, true, END_FINAL, COUNTS_OWN},     // up_unipose_frame_final_preds
    {UP_PROGRAM_FROM_FRAMES + 6, IN_FRAMES, false, END_FINAL, COUNTS_OWN},
};
// UniPose-LSTM (model/uniposeLSTM.py:67-138; the drop-in module unipose_amd/uniposeLSTM.py after checkpoint.load_folded).  The step
// programs are the module's per-frame path (batch_frames = False) for iter == 0 (LSTM_0) resp. iter > 0 with the caller's NCHW
// state; the clip programs its whole-clip unroll (_unroll_clip: batch_frames = batch_head = True), the flip test running the
// whole clip twice, each pass with its own recurrent state, so a flip program returns none.  The stream programs are the step
// programs with the state in the caller's buffer and up_heatmap_decode at the end; their NCHW heat-maps are optional.
// The serving programs (UP_PROGRAM_SERVE + 0 / + 1) are the stream programs for a batch whose samples are in different phases: BOTH
// gate convolutions at the plan's batch, the previous hidden state gathered per sample from the caller's pool straight into `zh`
// (up_lstm_state_gather, in place of STATE_IN and the copy behind it), ONE up_lstm_serve_fwd that picks the formula per sample and
// keeps the pool (in place of the two gate kernels, STATE_IN of the cell and both STATE_OUT).  At run time the lstm_0 convolution is
// skipped where no sample is first or idle; the copy of z, the gather and the lstm convolution where none continues.  A 3x3
// convolution mixes no images and a row's summation order depends on its position only, so lane b equals lane b of the stream
// program of its phase.  UP_PLAN_FLIP_ONE_PASS leaves them as they are.
// From frames (the rows numbered UP_PROGRAM_FROM_FRAMES + k, k the program the row otherwise equals): ONE crop launch stands in place
// of the layout pass(es) and, in the flip rows, fills the mirrored input too, which then stays alive through the first pass; the
// pooled centre map comes straight from the centre coordinates (up_center_pool and its clip forms), in the mirrored pass from the
// same coordinates through the _flip kernel.  The stream rows end in up_final_preds.  Every convolution launch is row k's.
static const Program LSTM_PROGRAMS[] = {
    {0, IN_NCHW, false, END_HEAT, COUNTS_PLAIN, STATE_NONE, STATE_NCHW},        // up_unipose_lstm_step, the first frame ...
    {1, IN_NCHW, false, END_HEAT, COUNTS_PLAIN, STATE_NCHW, STATE_NCHW},        // ... and a later one
    {2, IN_CLIP, false, END_HEAT, COUNTS_PLAIN, STATE_NONE, STATE_NCHW},        // up_unipose_lstm_clip
    {3, IN_CLIP, false, END_DECODE, COUNTS_PLAIN, STATE_NONE, STATE_NCHW},      // up_unipose_lstm_clip_keypoints
    {4, IN_CLIP, true, END_HEAT, COUNTS_FLIP},          // up_unipose_lstm_clip_flip
    {5, IN_CLIP, true, END_FINAL, COUNTS_FLIP},         // up_unipose_lstm_clip_final_preds with ...
    {6, IN_CLIP, false, END_FINAL, COUNTS_PLAIN},       // ... and without the flip test
    {7, IN_NCHW, false, END_DECODE, COUNTS_PLAIN, STATE_NONE, STATE_BUFFER},    // up_unipose_lstm_stream_keypoints, first ...
    {8, IN_NCHW, false, END_DECODE, COUNTS_PLAIN, STATE_BUFFER, STATE_BUFFER},  // ... and not
    {UP_PROGRAM_FROM_FRAMES + 2, IN_CLIP_FRAMES, false, END_HEAT, COUNTS_OWN, STATE_NONE, STATE_NCHW},   // up_unipose_lstm_clip_frame_heatmaps
    {UP_PROGRAM_FROM_FRAMES + 4, IN_CLIP_FRAMES, true, END_HEAT, COUNTS_OWN},
    {UP_PROGRAM_FROM_FRAMES + 5, IN_CLIP_FRAMES, true, END_FINAL, COUNTS_OWN},  // up_unipose_lstm_clip_frame_final_preds
    {UP_PROGRAM_FROM_FRAMES + 6, IN_CLIP_FRAMES, false, END_FINAL, COUNTS_OWN},
    {UP_PROGRAM_FROM_FRAMES + 7, IN_FRAMES, false, END_FINAL, COUNTS_OWN, STATE_NONE, STATE_BUFFER},     // up_unipose_lstm_stream_frame_final_preds
    {UP_PROGRAM_FROM_FRAMES + 8, IN_FRAMES, false, END_FINAL, COUNTS_OWN, STATE_BUFFER, STATE_BUFFER},
    {UP_PROGRAM_SERVE + 0, IN_NCHW, false, END_DECODE, COUNTS_OWN, STATE_POOL, STATE_POOL},     // up_unipose_lstm_serve_keypoints
    {UP_PROGRAM_SERVE + 1, IN_FRAMES, false, END_FINAL, COUNTS_OWN, STATE_POOL, STATE_POOL},    // up_unipose_lstm_serve_frame_final_preds
};
template <size_t N>
static int find(const Program (&table)[N], Input input, bool flip, Ending end, State from = STATE_NONE) {
    for (size_t i = 0; i < N; ++i)
        if (table[i].input == input && table[i].flip == flip && table[i].end == end && table[i].from == from) return (int)i;
    return -1;
}
template <size_t N>
static size_t program_workspace(const Program (&table)[N], const Plan* prog, int number) {
    for (size_t i = 0; i < N; ++i)
        if (table[i].number == number) return prog[i].ws_bytes;
    return 0;
}

// The flip rows of a plan created with UP_PLAN_FLIP_ONE_PASS: ONE trunk over 2 B images, image b the input and image B + b its
// mirror, both halves of one tensor (a Ref's `elems` reaches the second half: in the tensor's OWN elements, and the last convolution
// of a bf16 plan writes fp32 maps of rup32 lanes).  The layout passes are the two-pass form's, the crop's one launch fills both
// halves; the merge reads the two halves of the trunk's output.  The oracle is a plan of batch 2 B on cat(x, mirror(x)), whose
// launches these are; not bit-equal to the two-pass form wherever a convolution picks its kernel by the row count.
static void build_one_pass(Plan& p, const up_unipose_config& c, const Program& g, int dt) {
    const int n = c.batch;
    int h = c.height, w = c.width;
    const bool frames = g.input == IN_FRAMES;
    Ref x, m;
    x.id = p.tensor(2 * n, h, w, 4);
    m = x;
    m.elems = (size_t)n * h * w * 4;
    Op op;
    op.kind = frames ? CROP : TO_NHWC;
    op.out = x;
    if (frames) op.aux = m;
    op.ext = X;
    op.n = n; op.ch = 3;
    p.push(op);
    if (!frames) {
        op.kind = TO_NHWC_FLIP;
        op.out = m;
        p.push(op);
    }
    x = trunk(p, x, 2 * n, h, w, c.output_stride, c.out_channels, false, dt);
    m = x;
    m.elems = (size_t)n * h * w * p.tensors[x.id].c;
    op = Op();
    op.kind = MERGE;                             // into the caller's NCHW tensor, or in place on the first half
    op.in = x; op.aux = m;
    if (g.end == END_FINAL) op.out = x;
    op.ext = HEAT;
    op.n = n; op.ch = c.out_channels;
    p.push(op);
    if (g.end == END_FINAL) {
        op = Op();
        op.kind = FINAL;
        op.in = x;
        op.ext = HEAT;
        op.n = n; op.ch = c.out_channels;
        p.push(op);
    }
    p.layout();
}

static void build(Plan& p, const up_unipose_config& c, const Program& g, int dt, bool one_pass) {
    const int n = c.batch;
    int h = c.height, w = c.width;
    const bool frames = g.input == IN_FRAMES;
    p.grow_tail = dt == UP_DT_BF16;
    p.dt = dt;
    if (g.flip && one_pass) return build_one_pass(p, c, g, dt);
    // input NCHW -> NHWC, 3 -> 4 channels (ops.ToNHWC); from frames: the crop writes NHWC itself, and the mirror beside it
    Ref x, m;
    x.id = p.tensor(n, h, w, 4);
    if (frames && g.flip) m.id = p.tensor(n, h, w, 4);
    Op op;
    op.kind = frames ? CROP : TO_NHWC;
    op.out = x;
    op.aux = m;
    op.ext = X;
    op.n = n; op.ch = 3;
    p.push(op);
    x = trunk(p, x, n, h, w, c.output_stride, c.out_channels, false, dt);
    if (g.flip) {
        int h2 = c.height, w2 = c.width;
        if (!frames) {
            m.id = p.tensor(n, h2, w2, 4);
            op = Op();
            op.kind = TO_NHWC_FLIP;
            op.out = m;
            op.ext = X;
            op.n = n; op.ch = 3;
            p.push(op);
        }
        m = trunk(p, m, n, h2, w2, c.output_stride, c.out_channels, false, dt);
        op = Op();
        op.kind = MERGE;                         // straight into the caller's NCHW tensor, or ...
        op.in = x; op.aux = m;
        if (g.end == END_FINAL) op.out = x;      // ... in place: out == a with equal strides
        op.ext = HEAT;
        op.n = n; op.ch = c.out_channels;
        p.push(op);
    }
    if (g.end == END_UPSAMPLED) x = p.resample(BILINEAR, x, c.height, c.width);
    if (!(g.flip && g.end == END_HEAT)) {        // (there the merge has written the caller's heat-maps)
        op = Op();
        op.kind = g.end == END_FINAL ? FINAL : g.end == END_DECODE ? DECODE : g.end == END_PERSONS ? PERSONS : TO_NCHW;
        op.in = x;
        op.ext = HEAT;
        op.n = n; op.ch = c.out_channels;
        p.push(op);
    }
    p.layout();
}

struct LstmPass {
    Ref y, cells, hides;       // conv5's output and the state tensors, frame-major (T * B, h, w, .)
    int h = 0, w = 0;
};

// One pass of a video program up to conv5: the trunk once on the T * B frame-major images (T = 1 unless the input is a clip), the
// recurrence frame by frame on rows of frame-major state tensors, the head once on the T * B hidden states.  Stacked gate
// convolutions are named "lstm_0" / "lstm" (the plan builds their weights from the parts).  mirrored: the pass of the flip test.
// mirror: from frames, the mirrored input the first pass's crop launch fills for the second.
// one_pass (the flip rows of a plan created with UP_PLAN_FLIP_ONE_PASS): the ONE pass of the flip test over frames of 2 B images,
// image t * 2 B + b the plain sample and image t * 2 B + B + b its mirror.  The layout and pooling launches are the two passes' own
// through their _strided entries, each writing its half of every frame (the crop's one launch both); everything behind them is the
// plain pass at batch 2 B: the gate convolution of frame t runs on 2 B contiguous rows, so each half keeps its own state.
// dt: the trunk's storage.  Everything else stays fp32 tensors in a bf16 plan, as in the module (uniposeLSTM.py:166-168): the
// input pass, the hand-over, the state, the gate kernels and the head; Plan::conv picks each convolution's arithmetic.
static LstmPass lstm_pass(Plan& p, const up_unipose_lstm_config& c, const Program& g, bool mirrored, Ref& mirror, int dt,
                          bool one_pass = false) {
    const bool clip = g.input == IN_CLIP || g.input == IN_CLIP_FRAMES;
    const bool frames = g.input == IN_FRAMES || g.input == IN_CLIP_FRAMES;
    const int S = c.batch;                       // samples of the call; B: images per frame
    const int B = one_pass ? 2 * S : S, T = clip ? c.frames : 1, n = T * B, fi = one_pass ? B : 0;
    const int hc = c.num_classes + 1, cg = c.num_classes + 2, ldo = rup4(cg);
    int h = c.height, w = c.width;
    Ref x = mirror;
    if (!(frames && mirrored)) {
        x.id = p.tensor(n, h, w, 4);
        Op op;
        op.kind = frames ? (clip ? CLIP_CROP : CROP) : !clip ? TO_NHWC : mirrored ? CLIP_TO_NHWC_FLIP : CLIP_TO_NHWC;
        op.out = x;
        Ref half = x;                            // one pass: where the mirrored half of the first frame starts
        half.elems = (size_t)S * h * w * 4;
        if (frames && one_pass) {
            op.aux = half;
        } else if (frames && g.flip) {
            mirror.id = p.tensor(n, h, w, 4);
            op.aux = mirror;
        }
        op.ext = X;
        op.n = S; op.frames = T; op.ch = 3; op.fi = fi;
        p.push(op);
        if (one_pass && !frames) {
            op.kind = CLIP_TO_NHWC_FLIP;
            op.out = half;
            p.push(op);
        }
    }
    Ref heat = trunk(p, x, n, h, w, c.output_stride, hc, true, dt);
    // _AddCenter: the pooled centre map in the heat-maps' spare pad channel; (K + 1) % 4 == 0: a hand-over tensor of rup4(K + 2)
    // channels, zeros, the heat-maps copied in.  bf16 storage: the trunk's fp32 maps have rup32(K + 1) lanes, which the module slices
    // back to the fp32 layout (uniposeLSTM.py:119-124) — always the hand-over tensor, zeroed in every call (the gate convolution
    // reads all its lanes), the K + 1 real lanes copied in
    Ref z = heat;
    if (dt == UP_DT_BF16 || rup4(hc) == hc) {
        z.id = p.tensor(n, h, w, ldo);
        p.zero(z);
        p.copy(heat, p.tensors[heat.id].c, z, ldo, 0, (int64_t)n * h * w, hc);
    }
    const int ldz = p.tensors[z.id].c;       // == ldo either way
    {
        Op op;
        if (frames) op.kind = !clip ? CENTER_POOL : mirrored ? CLIP_CENTER_POOL_FLIP : CLIP_CENTER_POOL;
        else op.kind = !clip ? POOL : mirrored ? CLIP_POOL_FLIP : CLIP_POOL;
        op.out = z;
        op.ext = CENTER;
        op.n = S; op.frames = T; op.fi = fi;
        op.src_h = c.height; op.src_w = c.width; op.coff = hc;
        p.push(op);
        if (one_pass) {
            op.kind = frames ? CLIP_CENTER_POOL_FLIP : CLIP_POOL_FLIP;
            op.out.elems += (size_t)S * h * w * ldz;
            p.push(op);
        }
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
        op.n = B; op.ch = cg;
        op.out = ct; op.res = ht;
        if (g.from == STATE_POOL) {              // both gate convolutions, each sample's formula picked by the call's table
            op.kind = SERVE;
            op.in = p.conv("lstm_0", zt, B, h, w, ldz, cg, 3 * cg, 3, 1, 1, 1, 0, true);
            p.ops.back().when = ANY_FIRST;
            Ref zh;
            zh.id = p.tensor(B, h, w, ldz + ldo);
            p.copy(zt, ldz, zh, ldz + ldo, 0, (int64_t)frame, ldz);
            p.ops.back().when = ANY_NEXT;
            Op in;
            in.kind = GATHER;
            in.out = zh; in.coff = ldz;
            in.n = B;
            in.when = ANY_NEXT;
            p.push(in);
            op.aux = p.conv("lstm", zh, B, h, w, ldz + ldo, ldz + ldo, 4 * cg, 3, 1, 1, 1, 0, true);
            p.ops.back().when = ANY_NEXT;
        } else if (t == 0 && g.from == STATE_NONE) {    // LSTM_0 (uniposeLSTM.py:9-24)
            op.kind = LSTM0;
            op.in = p.conv("lstm_0", zt, B, h, w, ldz, cg, 3 * cg, 3, 1, 1, 1, 0, true);
        } else {                              // LSTM (uniposeLSTM.py:27-64): ONE convolution over cat(z, prev_hide)
            Ref ph, pc;
            if (g.from != STATE_NONE) {
                ph.id = p.tensor(B, h, w, ldo);
                pc.id = p.tensor(B, h, w, ldo);
                Op in;
                if (g.from == STATE_NCHW) {   // the caller's NCHW state (unipose._state: ToNHWC, pad channels zero)
                    in.kind = TO_NHWC;
                    in.n = B; in.ch = cg;
                    in.out = ph; in.ext = PREV_HIDE;
                    p.push(in);
                    in.out = pc; in.ext = PREV_CELL;
                    p.push(in);
                } else {                      // the caller's state buffer: the plan's own NHWC rows, pad channels as the plan left them
                    in.kind = STATE_IN;
                    in.out = ph; in.half = 0;
                    p.push(in);
                    in.out = pc; in.half = 1;
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
            p.copy(zt, ldz, zh, ldz + ldo, 0, (int64_t)frame, ldz);
            p.copy(ph, ldo, zh, ldz + ldo, ldz, (int64_t)frame, ldo);
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

static void build_lstm(Plan& p, const up_unipose_lstm_config& c, const Program& g, int dt, bool one_pass) {
    const bool clip = g.input == IN_CLIP || g.input == IN_CLIP_FRAMES;
    const int B = c.batch, T = clip ? c.frames : 1;
    const int hc = c.num_classes + 1, cg = c.num_classes + 2, ldo = rup4(cg);
    Ref mirror;
    p.dt = dt;
    p.grow_tail = dt == UP_DT_BF16;      // measured on the figures: every program of a bf16 plan needs less with it (B = 8, T = 5, 368 x 368:
                                         // 520 MB against 607 MB; the fp32 plan 1148 MB), so it is set; fp32 plans keep their layout
    LstmPass a = lstm_pass(p, c, g, false, mirror, dt, g.flip && one_pass);
    Op op;
    if (g.flip && one_pass) {                  // the two halves of every frame of conv5's output into a compact frame-major tensor
        const int ld = p.tensors[a.y.id].c;
        op.kind = CLIP_MERGE;
        op.in = a.y; op.aux = a.y;
        op.aux.elems += (size_t)B * a.h * a.w * ld;
        op.out.id = p.tensor(T * B, a.h, a.w, ld);
        op.n = B; op.frames = T; op.ch = hc;
        p.push(op);
        a.y = op.out;
    } else if (g.flip) {
        const LstmPass m = lstm_pass(p, c, g, true, mirror, dt);
        op.kind = MERGE;                       // in place (NHWC): out == a with equal strides; both passes are frame-major
        op.in = a.y; op.aux = m.y; op.out = a.y;
        op.n = T * B; op.ch = hc;
        p.push(op);
    }
    if (clip && g.end != END_HEAT) {           // a clip's joints: frame-major maps into batch-major results
        op = Op();
        op.kind = g.end == END_DECODE ? CLIP_DECODE : CLIP_FINAL;
        op.in = a.y;
        op.n = B; op.frames = T; op.ch = hc;
        p.push(op);
    }
    const size_t frame = (size_t)B * a.h * a.w;
    Ref cl = a.cells, hl = a.hides;            // the state of the last frame
    cl.elems += (T - 1) * frame * ldo;
    hl.elems += (T - 1) * frame * ldo;
    if (g.to == STATE_BUFFER || g.to == STATE_POOL) {      // the new state into the caller's buffer (SERVE has kept the pool), then the joints
        if (g.to == STATE_BUFFER) {
            op = Op();
            op.kind = STATE_OUT;
            op.in = hl; op.half = 0;
            p.push(op);
            op.in = cl; op.half = 1;
            p.push(op);
        }
        op = Op();
        op.kind = g.end == END_FINAL ? FINAL : DECODE;
        op.in = a.y;
        op.n = B; op.ch = hc;
        p.push(op);
    }
    if (g.end == END_HEAT || g.to == STATE_BUFFER || g.to == STATE_POOL) {
        op = Op();
        op.kind = clip ? CLIP_TO_NCHW : TO_NCHW;     // TO_NCHW is skipped where the caller passes no tensor (a stream's heat)
        op.in = a.y;
        op.ext = HEAT;
        op.n = B; op.frames = T; op.ch = hc;
        p.push(op);
    }
    if (g.to == STATE_NCHW) {
        op = Op();
        op.kind = TO_NCHW;
        op.n = B; op.ch = cg;
        op.in = cl; op.ext = CELL;
        p.push(op);
        op.in = hl; op.ext = HIDE;
        p.push(op);
    }
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
    float* pool = nullptr;           // GATHER / SERVE: the caller's pool (record stride in floats), its tables (host), and how many
    int64_t slot_stride = 0;         // of the samples are first or idle resp. continue (what the ops with a `when` are skipped by)
    int slots = 0, firsts = 0, nexts = 0;
    const int32_t* slot_host = nullptr;
    const int32_t* first_host = nullptr;
    const void* src = nullptr;       // CROP: the arguments of up_crop_to_nhwc
    int src_type = 0, frames = 0, src_h = 0, src_w = 0;
    const int32_t* frame_of = nullptr;
    const int32_t* valid_hw = nullptr;
    const double* crop_inv = nullptr;
    float border = 0.f, mean = 0.f, stdv = 0.f;
    const double* center_xy = nullptr;      // the centre-pool kinds: the arguments of up_center_pool
    double sigma = 0.0;
    const float* in(Ext e) const { return e == X ? x : e == CENTER ? center : e == PREV_HIDE ? prev_hide : prev_cell; }
    float* out(Ext e) const { return e == HEAT ? heat : e == CELL ? cell : hide; }
};

static int run(const Plan& p, const Io& io, unsigned char* ws, void* stream, const char* what) {
    auto ptr = [&](const Ref& r) -> float* {      // (a bf16 tensor travels through the same pointer arguments)
        return r.id < 0 ? nullptr : reinterpret_cast<float*>(ws + p.tensors[r.id].off + r.elems * p.tensors[r.id].elem);
    };
    auto dt = [](const Tensor& t) { return t.elem == 2 ? UP_DT_BF16 : UP_DT_F32; };
    static const Tensor none = {};
    for (const Op& op : p.ops) {
        // the tensors the op names, and the batch stride of NHWC maps read in place
        const Tensor& i = op.in.id < 0 ? none : p.tensors[op.in.id];
        const Tensor& o = op.out.id < 0 ? none : p.tensors[op.out.id];
        const int64_t image = (int64_t)i.h * i.w * i.c;
        int e = UP_OK;
        if ((op.when == ANY_FIRST && !io.firsts) || (op.when == ANY_NEXT && !io.nexts)) continue;
        switch (op.kind) {
        case TO_NHWC:
            e = up_nchw_to_nhwc(io.in(op.ext), ptr(op.out), op.n, op.ch, o.h, o.w, o.c, stream);
            break;
        case CONV: {
            const Conv& cv = p.convs[op.conv];
            up_conv_epilogue ep;
            memset(&ep, 0, sizeof(ep));
            ep.bias = cv.bias;
            ep.residual = ptr(op.res);
            ep.ldr = op.res.id >= 0 ? p.tensors[op.res.id].c : 0;
            ep.relu = cv.relu;
            if (cv.math == UP_MATH_F32)
                e = up_conv2d_fwd(&cv.d, ptr(op.in), cv.w_fwd, ptr(op.out), &ep, stream);
            else
                e = up_conv2d_fwd_bf16(&cv.d, ptr(op.in), reinterpret_cast<const uint16_t*>(cv.w_fwd), nullptr, ptr(op.out), &ep, cv.math,
                                       stream);
            break;
        }
        case MAXPOOL:
            e = up_maxpool3s2_fwd_t(ptr(op.in), i.c, ptr(op.out), o.c, reinterpret_cast<uint8_t*>(ptr(op.res)), op.n, i.h, i.w, i.c, o.h,
                                    o.w, dt(i), dt(o), stream);
            break;
        case BILINEAR:
            e = up_bilinear_fwd_t(ptr(op.in), i.c, ptr(op.out), o.c, op.n, i.h, i.w, i.c, o.h, o.w, dt(i), stream);
            break;
        case GAP:
            e = up_gap_fwd_t(ptr(op.in), i.c, ptr(op.out), op.n, i.h * i.w, i.c, dt(i), stream);
            break;
        case COPY: {      // the kernel moves 4-byte words: bf16 rows as half as many (strides, widths and offsets are multiples of 32)
            const int per = (int)(4 / i.elem);
            e = up_copy2d(ptr(op.in), op.lds / per, ptr(op.out), op.ldd / per, op.rows, op.ch / per, stream);
            break;
        }
        case ZERO:
            if (hipMemsetAsync(ptr(op.out), 0, o.bytes, as_stream(stream)) != hipSuccess) e = check_launch(what);
            break;
        case TO_NCHW:
            if (io.out(op.ext)) e = up_nhwc_to_nchw(ptr(op.in), i.c, io.out(op.ext), op.n, op.ch, i.h, i.w, stream);
            break;
        case DECODE:
            e = up_heatmap_decode(ptr(op.in), image, 1, i.c, op.n, op.ch, i.h, i.w, io.dec_h, io.dec_w, io.idx, io.preds, io.maxvals, stream);
            break;
        case PERSONS:
            e = up_persons_decode(ptr(op.in), image, 1, i.c, op.n, op.ch, i.h, i.w, io.box_ch0, io.joint_ch0, io.njoints, io.max_persons,
                                  io.count, io.status, io.kpts, stream);
            break;
        case TO_NHWC_FLIP:
            e = up_nchw_to_nhwc_flip(io.in(op.ext), ptr(op.out), op.n, op.ch, o.h, o.w, o.c, stream);
            break;
        case CROP:
            e = up_crop_to_nhwc(io.src, io.src_type, io.frames, io.src_h, io.src_w, op.ch, io.frame_of, io.valid_hw, io.crop_inv, op.n,
                                io.border, io.mean, io.stdv, ptr(op.out), ptr(op.aux), o.h, o.w, o.c, stream);
            break;
        case MERGE:
            if (op.out.id >= 0)
                e = up_flip_merge(ptr(op.in), ptr(op.aux), image, 1, i.c, op.n, op.ch, i.h, i.w, io.perm, ptr(op.out), image, 1, i.c, stream);
            else
                e = up_flip_merge(ptr(op.in), ptr(op.aux), image, 1, i.c, op.n, op.ch, i.h, i.w, io.perm, io.out(op.ext),
                                  (int64_t)op.ch * i.h * i.w, (int64_t)i.h * i.w, 1, stream);
            break;
        case FINAL:
            e = up_final_preds(ptr(op.in), image, 1, i.c, op.n, op.ch, i.h, i.w, io.res0, io.res1, io.inv, io.preds, io.coords, io.maxvals,
                               stream);
            break;
        case POOL:
            e = up_avgpool9s8_fwd(io.in(op.ext), ptr(op.out), o.c, op.coff, op.n, op.src_h, op.src_w, o.h, o.w, stream);
            break;
        case CLIP_POOL:
            if (op.fi)
                e = up_clip_avgpool9s8_fwd_strided(io.in(op.ext), ptr(op.out), o.c, op.coff, op.n, op.frames, op.src_h, op.src_w, o.h, o.w,
                                                   op.fi, 0, stream);
            else
                e = up_clip_avgpool9s8_fwd(io.in(op.ext), ptr(op.out), o.c, op.coff, op.n, op.frames, op.src_h, op.src_w, o.h, o.w, stream);
            break;
        case LSTM0:
            e = up_lstm0_fwd(ptr(op.in), i.c, ptr(op.out), ptr(op.res), o.c, (int64_t)op.n * i.h * i.w, op.ch, stream);
            break;
        case LSTM:
            e = up_lstm_fwd(ptr(op.in), i.c, ptr(op.aux), p.tensors[op.aux.id].c, ptr(op.out), ptr(op.res), o.c, (int64_t)op.n * i.h * i.w,
                            op.ch, stream);
            break;
        case CLIP_TO_NHWC:
            if (op.fi)
                e = up_clip_nchw_to_nhwc_strided(io.in(op.ext), ptr(op.out), op.n, op.frames, op.ch, o.h, o.w, o.c, op.fi, 0, stream);
            else
                e = up_clip_nchw_to_nhwc(io.in(op.ext), ptr(op.out), op.n, op.frames, op.ch, o.h, o.w, o.c, stream);
            break;
        case CLIP_TO_NCHW:
            e = up_clip_nhwc_to_nchw(ptr(op.in), i.c, io.out(op.ext), op.n, op.frames, op.ch, i.h, i.w, stream);
            break;
        case CLIP_TO_NHWC_FLIP:
            if (op.fi)
                e = up_clip_nchw_to_nhwc_flip_strided(io.in(op.ext), ptr(op.out), op.n, op.frames, op.ch, o.h, o.w, o.c, op.fi, 0, stream);
            else
                e = up_clip_nchw_to_nhwc_flip(io.in(op.ext), ptr(op.out), op.n, op.frames, op.ch, o.h, o.w, o.c, stream);
            break;
        case CLIP_POOL_FLIP:
            if (op.fi)
                e = up_clip_avgpool9s8_flip_fwd_strided(io.in(op.ext), ptr(op.out), o.c, op.coff, op.n, op.frames, op.src_h, op.src_w, o.h,
                                                        o.w, op.fi, 0, stream);
            else
                e = up_clip_avgpool9s8_flip_fwd(io.in(op.ext), ptr(op.out), o.c, op.coff, op.n, op.frames, op.src_h, op.src_w, o.h, o.w,
                                                stream);
            break;
        case CLIP_MERGE:       // frame t: images t * 2 B + b of `in` and of `aux` (B images on) into image t * B + b of `out`
            e = up_clip_flip_merge(ptr(op.in), ptr(op.aux), 2 * op.n * image, image, 1, i.c, op.n, op.frames, op.ch, i.h, i.w, io.perm,
                                   ptr(op.out), op.n * image, image, 1, i.c, stream);
            break;
        case CLIP_DECODE:
            e = up_clip_heatmap_decode(ptr(op.in), image, 1, i.c, op.n, op.frames, op.ch, i.h, i.w, io.dec_h, io.dec_w, io.idx, io.preds,
                                       io.maxvals, stream);
            break;
        case CLIP_FINAL:
            e = up_clip_final_preds(ptr(op.in), image, 1, i.c, op.n, op.frames, op.ch, i.h, i.w, io.res0, io.res1, io.inv, io.preds,
                                    io.coords, io.maxvals, stream);
            break;
        case CLIP_CROP:
            if (op.fi)
                e = up_clip_crop_to_nhwc_strided(io.src, io.src_type, io.frames, io.src_h, io.src_w, op.ch, io.frame_of, io.valid_hw,
                                                 io.crop_inv, op.n, op.frames, io.border, io.mean, io.stdv, ptr(op.out), ptr(op.aux), o.h,
                                                 o.w, o.c, op.fi, 0, stream);
            else
                e = up_clip_crop_to_nhwc(io.src, io.src_type, io.frames, io.src_h, io.src_w, op.ch, io.frame_of, io.valid_hw, io.crop_inv,
                                         op.n, op.frames, io.border, io.mean, io.stdv, ptr(op.out), ptr(op.aux), o.h, o.w, o.c, stream);
            break;
        case CENTER_POOL:
            e = up_center_pool(io.center_xy, io.sigma, ptr(op.out), o.c, op.coff, op.n, op.src_h, op.src_w, o.h, o.w, stream);
            break;
        case CLIP_CENTER_POOL:
            if (op.fi)
                e = up_clip_center_pool_strided(io.center_xy, io.sigma, ptr(op.out), o.c, op.coff, op.n, op.frames, op.src_h, op.src_w, o.h,
                                                o.w, op.fi, 0, stream);
            else
                e = up_clip_center_pool(io.center_xy, io.sigma, ptr(op.out), o.c, op.coff, op.n, op.frames, op.src_h, op.src_w, o.h, o.w,
                                        stream);
            break;
        case CLIP_CENTER_POOL_FLIP:
            if (op.fi)
                e = up_clip_center_pool_flip_strided(io.center_xy, io.sigma, ptr(op.out), o.c, op.coff, op.n, op.frames, op.src_h, op.src_w,
                                                     o.h, o.w, op.fi, 0, stream);
            else
                e = up_clip_center_pool_flip(io.center_xy, io.sigma, ptr(op.out), o.c, op.coff, op.n, op.frames, op.src_h, op.src_w, o.h, o.w,
                                             stream);
            break;
        case STATE_IN:                         // whole padded rows: the pad channels stay the zeros the plan wrote
            e = up_copy2d(io.state + op.half * io.state_half, o.c, ptr(op.out), o.c, (int64_t)o.n * o.h * o.w, o.c, stream);
            break;
        case STATE_OUT:
            e = up_copy2d(ptr(op.in), i.c, io.state + op.half * io.state_half, i.c, (int64_t)i.n * i.h * i.w, i.c, stream);
            break;
        case GATHER:                           // the hidden states into the lanes of `zh` behind z: all o.c - coff of them
            e = up_lstm_state_gather(io.pool, io.slot_stride, io.slots, io.slot_host, io.first_host, op.n, (int64_t)o.h * o.w,
                                     o.c - op.coff, ptr(op.out), o.c, op.coff, stream);
            break;
        case SERVE:                            // a gate tensor whose convolution was skipped is not passed
            e = up_lstm_serve_fwd(io.firsts ? ptr(op.in) : nullptr, i.c, io.nexts ? ptr(op.aux) : nullptr, p.tensors[op.aux.id].c, io.pool,
                                  io.slot_stride, io.slots, io.slot_host, io.first_host, ptr(op.out), ptr(op.res), o.c, op.n,
                                  (int64_t)i.h * i.w, op.ch, stream);
            break;
        }
        if (e) return e;
    }
    return UP_OK;
}

// ---- the weights of a plan --------------------------------------------------------------------------------------------------------
// Stored once per distinct parameter and shared by every program, and within one (wasp.conv2 is applied twice).  The ConvLSTM
// gate convolutions of the video plan are set part by part under their state_dict names and stacked by the plan
// (modules.LSTM_0.forward / modules.LSTM.stacked): along the output channels, the x / h parts' input channels padded to rup4,
// each gate bias the fp32 sum bx + bh.
struct Store {                 // one packed forward weight image (+ bias)
    std::string name;          // a state_dict prefix, or "lstm_0" / "lstm" for the stacked gate convolutions
    up_conv_desc d;            // descriptor of its first use (the packed image depends on K, C, Cp, R, S only)
    bool has_bias = false;
    bool b16 = false;          // the bf16 hi plane of up_pack_weights_bf16 (a launch of up_conv2d_fwd_bf16, whatever its tensors' type),
                               // else the fp32 image
    float* w_fwd = nullptr;
    float* bias = nullptr;     // fp32 in either storage
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
struct Weights {
    std::vector<Store> stores;
    std::vector<Entry> entries;
    uint16_t* lo = nullptr;    // bf16 storage: where up_pack_weights_bf16 puts the lo plane it always writes beside the hi plane.  No
                               // launch of the plan reads it (only UP_MATH_BF16X3 does), so ONE buffer of the largest image serves
                               // every store, whatever the order or the streams of the set_conv calls

    int store_of(const std::string& name) const {
        for (size_t s = 0; s < stores.size(); ++s)
            if (stores[s].name == name) return (int)s;
        return -1;
    }
    // One store per distinct name of the programs, in device memory, and every convolution bound to its own.  cg: channels of one
    // gate of the stacked convolutions.  false: out of device memory (release() takes what was allocated).
    bool bind(Plan* progs, size_t count, int cg) {
        for (size_t f = 0; f < count; ++f)
            for (const Conv& cv : progs[f].convs) {
                if (store_of(cv.name) >= 0) continue;
                Store st;
                st.name = cv.name;
                st.d = cv.d;
                st.has_bias = cv.has_bias;
                st.b16 = cv.math != UP_MATH_F32;
                st.parts = cv.name == "lstm_0" ? 3 : cv.name == "lstm" ? 8 : 0;
                stores.push_back(st);
            }
        bool ok = true;
        size_t lo_elems = 0;
        for (Store& st : stores) {
            const size_t image = (size_t)st.d.K * st.d.R * st.d.S * st.d.Cp;
            if (st.b16) lo_elems = std::max(lo_elems, image);
            st.w_fwd = static_cast<float*>(dev_alloc(image * (st.b16 ? sizeof(uint16_t) : sizeof(float))));
            if (st.has_bias) st.bias = static_cast<float*>(dev_alloc((size_t)st.d.K * sizeof(float)));
            ok = ok && st.w_fwd && (!st.has_bias || st.bias);
            if (st.parts) {
                st.stage_w = static_cast<float*>(dev_alloc((size_t)st.d.K * st.d.C * st.d.R * st.d.S * sizeof(float)));
                st.stage_b = static_cast<float*>(dev_alloc((size_t)st.parts * cg * sizeof(float)));
                ok = ok && st.stage_w && st.stage_b;
            }
        }
        if (lo_elems) {
            lo = static_cast<uint16_t*>(dev_alloc(lo_elems * sizeof(uint16_t)));
            ok = ok && lo;
        }
        for (size_t f = 0; f < count; ++f)
            for (Conv& cv : progs[f].convs) {
                const Store& st = stores[store_of(cv.name)];
                cv.w_fwd = st.w_fwd;
                cv.bias = st.bias;
            }
        return ok;
    }
    void list(const std::string& name, int store, int part, int k, int c, int r, bool bias) {
        Entry e;
        e.name = name;
        e.oihw[0] = k; e.oihw[1] = c; e.oihw[2] = r; e.oihw[3] = r;
        e.has_bias = bias;
        e.store = store;
        e.part = part;
        entries.push_back(e);
    }
    void release() {
        for (Store& st : stores) {
            dev_free(st.w_fwd);
            dev_free(st.bias);
            dev_free(st.stage_w);
            dev_free(st.stage_b);
        }
        dev_free(lo);
    }
};

// The listing both plans answer with (`w` is NULL where the plan is); `what` names the C function in the refusal.
static int num_convs(const Weights* w) { return w ? (int)w->entries.size() : UP_ERR_INVALID; }
static const char* conv_name(const Weights* w, int i) { return (w && i >= 0 && i < (int)w->entries.size()) ? w->entries[i].name.c_str() : ""; }
static int conv_shape(const Weights* w, int i, int32_t* oihw, int32_t* has_bias, const char* what) {
    UP_REQUIRE(w && oihw && i >= 0 && i < (int)w->entries.size(), UP_ERR_INVALID, "%s: bad argument", what);
    const Entry& e = w->entries[i];
    memcpy(oihw, e.oihw, sizeof(e.oihw));
    if (has_bias) *has_bias = e.has_bias ? 1 : 0;
    return UP_OK;
}
static int set_conv_check(const Weights* w, int i, const float* w_oihw, const float* bias, const char* what) {
    UP_REQUIRE(w && w_oihw && i >= 0 && i < (int)w->entries.size(), UP_ERR_INVALID, "%s: bad argument", what);
    const Entry& en = w->entries[i];
    UP_REQUIRE((bias != nullptr) == en.has_bias, UP_ERR_INVALID, "%s: %s %s a bias (folded network)", what, en.name.c_str(),
               en.has_bias ? "needs" : "has no");
    return UP_OK;
}
// an OIHW image into its store, in the store's type (a stacked one: stacked in fp32 first, rounded once, like ops._packed_bf16)
static int pack(const Weights& w, const Store& st, const float* w_oihw, void* stream) {
    if (st.b16) return up_pack_weights_bf16(&st.d, w_oihw, reinterpret_cast<uint16_t*>(st.w_fwd), w.lo, nullptr, nullptr, stream);
    return up_pack_weights(&st.d, w_oihw, st.w_fwd, nullptr, stream);
}
// an entry that is a whole parameter: packed into its store; every listing of the name is set with it
static int set_conv_whole(Weights& w, int i, const float* w_oihw, const float* bias, void* stream) {
    const Entry& en = w.entries[i];
    const Store& st = w.stores[en.store];
    if (int e = pack(w, st, w_oihw, stream)) return e;
    if (bias)
        if (int e = up_copy2d(bias, st.d.K, st.bias, st.d.K, 1, st.d.K, stream)) return e;
    for (Entry& other : w.entries)
        if (other.name == en.name) other.set = true;
    return UP_OK;
}

// ---- one call -----------------------------------------------------------------------------------------------------------------------
// Weights set, a workspace of `need` bytes, then the launches.  setter: the function the "never set" refusal points to;
// ws_code: what a too-small or misaligned workspace returns (the two plans differ).
static int launch(const Weights& w, const char* setter, const Plan& prog, size_t need, int ws_code, const Io& io, void* workspace,
                  size_t ws_bytes, void* stream, const char* what) {
    for (const Entry& e : w.entries)
        UP_REQUIRE(e.set, UP_ERR_INVALID, "%s: weights of %s were never set (%s)", what, e.name.c_str(), setter);
    UP_REQUIRE(ws_bytes >= need && (reinterpret_cast<uintptr_t>(workspace) & 255) == 0, ws_code,
               "%s: workspace of %zu bytes (256-byte aligned) needed, got %zu", what, need, ws_bytes);
    return run(prog, io, static_cast<unsigned char*>(workspace), stream, what);
}
// the channel permutation of a flip-test call over C `noun` channels: refused before the first launch of the program
static int perm_ok(int C, const char* noun, const int32_t* perm, const char* what) {
    UP_REQUIRE(C <= 256, UP_ERR_UNSUPPORTED, "%s: %d %s channels (up_flip_merge takes up to 256)", what, C, noun);
    for (int j = 0; j < C; ++j)
        UP_REQUIRE(perm[j] >= 0 && perm[j] < C, UP_ERR_INVALID, "%s: perm[%d] = %d outside 0..%d", what, j, (int)perm[j], C - 1);
    return UP_OK;
}
// the grid of a decode: the heat-maps' own (three ceil-halvings of the H x W input) or the input's
static int grid_ok(int out_h, int out_w, int H, int W, const char* what) {
    const int h = (H - 1) / 8 + 1, w = (W - 1) / 8 + 1;
    UP_REQUIRE((out_h == h && out_w == w) || (out_h == H && out_w == W), UP_ERR_INVALID,
               "%s: a %d x %d grid; the plan decodes on the heat-maps' %d x %d or the input's %d x %d", what, out_h, out_w, h, w, H, W);
    return UP_OK;
}

}  // namespace plan
}  // namespace up

using namespace up;
using up::plan::Plan;

// ---- the image plan -----------------------------------------------------------------------------------------------------------------
static const size_t IMAGE_FORMS = sizeof(plan::IMAGE_PROGRAMS) / sizeof(plan::IMAGE_PROGRAMS[0]);

struct up_unipose_plan {
    up_unipose_config cfg;
    Plan prog[IMAGE_FORMS];    // as IMAGE_PROGRAMS lists them
    int dtype = UP_DT_F32;     // the storage behind the stem: activations in the workspace and the packed weight images
    int flags = 0;             // UP_PLAN_*: how the flip rows are built
    plan::Weights w;           // the listed convolutions are those of program 0: the 116 of the forward, wasp.conv2 twice
    size_t ws_bytes = 0;       // the largest of the programs that count toward it, and ...
    size_t flip_ws_bytes = 0;  // ... toward the flip test's
};

extern "C" int up_unipose_plan_create(const up_unipose_config* cfg, up_unipose_plan** out) {
    return up_unipose_plan_create_t(cfg, UP_DT_F32, out);
}

extern "C" int up_unipose_plan_dtype(const up_unipose_plan* pl) { return pl ? pl->dtype : UP_ERR_INVALID; }

extern "C" int up_unipose_plan_create_t(const up_unipose_config* cfg, int dtype, up_unipose_plan** out) {
    return up_unipose_plan_create_ex(cfg, dtype, 0, out);
}

extern "C" int up_unipose_plan_flags(const up_unipose_plan* pl) { return pl ? pl->flags : UP_ERR_INVALID; }

extern "C" int up_unipose_plan_create_ex(const up_unipose_config* cfg, int dtype, int flags, up_unipose_plan** out) {
    UP_REQUIRE(cfg && out, UP_ERR_INVALID, "unipose_plan_create: null argument");
    UP_REQUIRE(dtype == UP_DT_F32 || dtype == UP_DT_BF16, UP_ERR_INVALID, "unipose_plan_create: storage type %d (UP_DT_F32 or UP_DT_BF16)",
               dtype);
    UP_REQUIRE((flags & ~UP_PLAN_FLIP_ONE_PASS) == 0, UP_ERR_INVALID, "unipose_plan_create: flags %d (UP_PLAN_FLIP_ONE_PASS or 0)", flags);
    UP_REQUIRE(cfg->batch > 0 && cfg->height >= 32 && cfg->width >= 32 && cfg->out_channels > 0, UP_ERR_INVALID,
               "unipose_plan_create: batch %d, input %dx%d, %d output channels", cfg->batch, cfg->height, cfg->width, cfg->out_channels);
    UP_REQUIRE(cfg->output_stride == 16 || cfg->output_stride == 8, UP_ERR_UNSUPPORTED,
               "unipose_plan_create: output stride %d (the reference builds 16 and 8, resnet.py:49-58)", cfg->output_stride);
    up_unipose_plan* pl = new (std::nothrow) up_unipose_plan();
    UP_REQUIRE(pl, UP_ERR_INVALID, "unipose_plan_create: out of host memory");
    pl->cfg = *cfg;
    pl->dtype = dtype;
    pl->flags = flags;
    for (size_t f = 0; f < IMAGE_FORMS; ++f) {
        const plan::Program& g = plan::IMAGE_PROGRAMS[f];
        plan::build(pl->prog[f], pl->cfg, g, dtype, (flags & UP_PLAN_FLIP_ONE_PASS) != 0);
        if (g.counts == plan::COUNTS_PLAIN) pl->ws_bytes = std::max(pl->ws_bytes, pl->prog[f].ws_bytes);
        if (g.counts == plan::COUNTS_FLIP) pl->flip_ws_bytes = std::max(pl->flip_ws_bytes, pl->prog[f].ws_bytes);
    }
    const bool ok = pl->w.bind(pl->prog, IMAGE_FORMS, 0);
    for (const plan::Conv& cv : pl->prog[0].convs) pl->w.list(cv.name, pl->w.store_of(cv.name), -1, cv.d.K, cv.d.C, cv.d.R, cv.has_bias);
    if (!ok) {
        up_unipose_plan_destroy(pl);
        UP_REQUIRE(false, UP_ERR_INVALID, "unipose_plan_create: out of device memory");
    }
    *out = pl;
    return UP_OK;
}

extern "C" void up_unipose_plan_destroy(up_unipose_plan* pl) {
    if (!pl) return;
    pl->w.release();
    delete pl;
}

extern "C" int up_unipose_plan_num_convs(const up_unipose_plan* pl) { return plan::num_convs(pl ? &pl->w : nullptr); }

extern "C" const char* up_unipose_plan_conv_name(const up_unipose_plan* pl, int i) { return plan::conv_name(pl ? &pl->w : nullptr, i); }

extern "C" int up_unipose_plan_conv_shape(const up_unipose_plan* pl, int i, int32_t* oihw, int32_t* has_bias) {
    return plan::conv_shape(pl ? &pl->w : nullptr, i, oihw, has_bias, "unipose_plan_conv_shape");
}

extern "C" int up_unipose_plan_set_conv(up_unipose_plan* pl, int i, const float* w_oihw, const float* bias, void* stream) {
    if (int e = plan::set_conv_check(pl ? &pl->w : nullptr, i, w_oihw, bias, "unipose_plan_set_conv")) return e;
    return plan::set_conv_whole(pl->w, i, w_oihw, bias, stream);
}

extern "C" size_t up_unipose_plan_workspace(const up_unipose_plan* pl) { return pl ? pl->ws_bytes : 0; }

extern "C" size_t up_unipose_plan_flip_workspace(const up_unipose_plan* pl) { return pl ? pl->flip_ws_bytes : 0; }

extern "C" size_t up_unipose_plan_program_workspace(const up_unipose_plan* pl, int program) {
    return pl ? plan::program_workspace(plan::IMAGE_PROGRAMS, pl->prog, program) : 0;
}

// the program of an entry's arguments, ready and run: a too-small workspace is UP_ERR_INVALID from this plan
static int launch(up_unipose_plan* pl, plan::Input input, bool flip, plan::Ending end, const plan::Io& io, void* workspace, size_t ws_bytes,
                  void* stream, const char* what) {
    const Plan& prog = pl->prog[plan::find(plan::IMAGE_PROGRAMS, input, flip, end)];
    return plan::launch(pl->w, "up_unipose_plan_set_conv", prog, prog.ws_bytes, UP_ERR_INVALID, io, workspace, ws_bytes, stream, what);
}

extern "C" int up_unipose_forward(up_unipose_plan* pl, const float* x_nchw, float* heat_nchw, void* workspace, size_t ws_bytes,
                                  void* stream) {
    UP_REQUIRE(pl && x_nchw && heat_nchw && workspace, UP_ERR_INVALID, "unipose_forward: null argument");
    plan::Io io;
    io.x = x_nchw;
    io.heat = heat_nchw;
    return launch(pl, plan::IN_NCHW, false, plan::END_HEAT, io, workspace, ws_bytes, stream, "unipose_forward");
}

extern "C" int up_unipose_forward_upsampled(up_unipose_plan* pl, const float* x_nchw, float* heat_nchw, void* workspace,
                                            size_t ws_bytes, void* stream) {
    UP_REQUIRE(pl && x_nchw && heat_nchw && workspace, UP_ERR_INVALID, "unipose_forward_upsampled: null argument");
    plan::Io io;
    io.x = x_nchw;
    io.heat = heat_nchw;
    return launch(pl, plan::IN_NCHW, false, plan::END_UPSAMPLED, io, workspace, ws_bytes, stream, "unipose_forward_upsampled");
}

extern "C" int up_unipose_keypoints(up_unipose_plan* pl, const float* x_nchw, int out_h, int out_w, int32_t* idx, float* preds_xy,
                                    float* maxvals, void* workspace, size_t ws_bytes, void* stream) {
    UP_REQUIRE(pl && x_nchw && preds_xy && maxvals && workspace, UP_ERR_INVALID, "unipose_keypoints: null argument");
    if (int e = plan::grid_ok(out_h, out_w, pl->cfg.height, pl->cfg.width, "unipose_keypoints")) return e;
    plan::Io io;
    io.x = x_nchw;
    io.dec_h = out_h;
    io.dec_w = out_w;
    io.idx = idx;
    io.preds = preds_xy;
    io.maxvals = maxvals;
    return launch(pl, plan::IN_NCHW, false, plan::END_DECODE, io, workspace, ws_bytes, stream, "unipose_keypoints");
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
    plan::Io io;
    io.x = x_nchw;
    io.box_ch0 = box_ch0;
    io.joint_ch0 = joint_ch0;
    io.njoints = njoints;
    io.max_persons = max_persons;
    io.count = count;
    io.status = status;
    io.kpts = kpts;
    return launch(pl, plan::IN_NCHW, false, plan::END_PERSONS, io, workspace, ws_bytes, stream, "unipose_persons");
}

extern "C" int up_unipose_flip_forward(up_unipose_plan* pl, const float* x_nchw, const int32_t* perm_host, float* heat_nchw,
                                       void* workspace, size_t ws_bytes, void* stream) {
    UP_REQUIRE(pl && x_nchw && perm_host && heat_nchw && workspace, UP_ERR_INVALID, "unipose_flip_forward: null argument");
    if (int e = plan::perm_ok(pl->cfg.out_channels, "output", perm_host, "unipose_flip_forward")) return e;
    plan::Io io;
    io.x = x_nchw;
    io.perm = perm_host;
    io.heat = heat_nchw;
    return launch(pl, plan::IN_NCHW, true, plan::END_HEAT, io, workspace, ws_bytes, stream, "unipose_flip_forward");
}

extern "C" int up_unipose_final_preds(up_unipose_plan* pl, const float* x_nchw, const int32_t* perm_host, const double* inv, int res0,
                                      int res1, float* preds_xy, float* coords_xy, float* maxvals, void* workspace, size_t ws_bytes,
                                      void* stream) {
    UP_REQUIRE(pl && x_nchw && preds_xy && maxvals && workspace, UP_ERR_INVALID, "unipose_final_preds: null argument");
    UP_REQUIRE(res0 > 0 && res1 > 0, UP_ERR_INVALID, "unipose_final_preds: res %d, %d", res0, res1);
    if (perm_host)
        if (int e = plan::perm_ok(pl->cfg.out_channels, "output", perm_host, "unipose_final_preds")) return e;
    plan::Io io;
    io.x = x_nchw;
    io.perm = perm_host;
    io.inv = inv;
    io.res0 = res0;
    io.res1 = res1;
    io.preds = preds_xy;
    io.coords = coords_xy;
    io.maxvals = maxvals;
    return launch(pl, plan::IN_NCHW, perm_host != nullptr, plan::END_FINAL, io, workspace, ws_bytes, stream, "unipose_final_preds");
}

// From source frames: the crop of up_crop_to_nhwc in front of the same programs.  Its own refusals (source type, sizes,
// frame_of == NULL with F != samples, std) come from its wrapper, which is the program's first launch: nothing runs before it.
// samples: the image plan's batch, the video plan's B * T (a clip) or B (a stream).
static int frame_io(int samples, plan::Io& io, const void* src_hwc, int src_type, int F, int Hs, int Ws,
                    const int32_t* frame_of, const int32_t* valid_hw, const double* crop_inv, float border, float mean, float stdv,
                    const char* what) {
    UP_REQUIRE(src_hwc && crop_inv, UP_ERR_INVALID, "%s: null source frames or crop maps", what);
    UP_REQUIRE(src_type == UP_PIX_U8 || src_type == UP_PIX_F32, UP_ERR_INVALID, "%s: source type %d", what, src_type);
    UP_REQUIRE(F > 0 && Hs > 0 && Ws > 0, UP_ERR_INVALID, "%s: %d frames of %d x %d", what, F, Hs, Ws);
    UP_REQUIRE(frame_of || F == samples, UP_ERR_INVALID, "%s: no frame_of with %d frames for a batch of %d", what, F, samples);
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
    if (int e = frame_io(pl->cfg.batch, io, src_hwc, src_type, F, Hs, Ws, frame_of, valid_hw, crop_inv, border, mean, stdv,
                         "unipose_frame_heatmaps"))
        return e;
    if (perm_host)
        if (int e = plan::perm_ok(pl->cfg.out_channels, "output", perm_host, "unipose_frame_heatmaps")) return e;
    io.perm = perm_host;
    io.heat = heat_nchw;
    return launch(pl, plan::IN_FRAMES, perm_host != nullptr, plan::END_HEAT, io, workspace, ws_bytes, stream, "unipose_frame_heatmaps");
}

extern "C" int up_unipose_frame_final_preds(up_unipose_plan* pl, const void* src_hwc, int src_type, int F, int Hs, int Ws,
                                            const int32_t* frame_of, const int32_t* valid_hw, const double* crop_inv, float border,
                                            float mean, float stdv, const int32_t* perm_host, const double* inv, int res0, int res1,
                                            float* preds_xy, float* coords_xy, float* maxvals, void* workspace, size_t ws_bytes,
                                            void* stream) {
    UP_REQUIRE(pl && preds_xy && maxvals && workspace, UP_ERR_INVALID, "unipose_frame_final_preds: null argument");
    UP_REQUIRE(res0 > 0 && res1 > 0, UP_ERR_INVALID, "unipose_frame_final_preds: res %d, %d", res0, res1);
    plan::Io io;
    if (int e = frame_io(pl->cfg.batch, io, src_hwc, src_type, F, Hs, Ws, frame_of, valid_hw, crop_inv, border, mean, stdv,
                         "unipose_frame_final_preds"))
        return e;
    if (perm_host)
        if (int e = plan::perm_ok(pl->cfg.out_channels, "output", perm_host, "unipose_frame_final_preds")) return e;
    io.perm = perm_host;
    io.inv = inv;
    io.res0 = res0;
    io.res1 = res1;
    io.preds = preds_xy;
    io.coords = coords_xy;
    io.maxvals = maxvals;
    return launch(pl, plan::IN_FRAMES, perm_host != nullptr, plan::END_FINAL, io, workspace, ws_bytes, stream, "unipose_frame_final_preds");
}

// ---- the video plan -----------------------------------------------------------------------------------------------------------------
static const size_t LSTM_FORMS = sizeof(plan::LSTM_PROGRAMS) / sizeof(plan::LSTM_PROGRAMS[0]);

struct up_unipose_lstm_plan {
    up_unipose_lstm_config cfg;
    Plan prog[LSTM_FORMS];     // as LSTM_PROGRAMS lists them
    int dtype = UP_DT_F32;     // the trunk's storage: its activations and packed weight images; state, head and all I/O are fp32
    int flags = 0;             // UP_PLAN_*: how the flip rows are built
    plan::Weights w;
    size_t ws_bytes = 0;       // the largest of the programs without the flip test
    size_t flip_ws_bytes = 0;  // the largest of those with it
    size_t state_half = 0;     // elements of one (B, h, w, rup4(K + 2)) state tensor in a stream's buffer, a multiple of 64
};

extern "C" int up_unipose_lstm_plan_create(const up_unipose_lstm_config* cfg, up_unipose_lstm_plan** out) {
    return up_unipose_lstm_plan_create_t(cfg, UP_DT_F32, out);
}

extern "C" int up_unipose_lstm_plan_dtype(const up_unipose_lstm_plan* pl) { return pl ? pl->dtype : UP_ERR_INVALID; }

extern "C" int up_unipose_lstm_plan_create_t(const up_unipose_lstm_config* cfg, int dtype, up_unipose_lstm_plan** out) {
    return up_unipose_lstm_plan_create_ex(cfg, dtype, 0, out);
}

extern "C" int up_unipose_lstm_plan_flags(const up_unipose_lstm_plan* pl) { return pl ? pl->flags : UP_ERR_INVALID; }

extern "C" int up_unipose_lstm_plan_create_ex(const up_unipose_lstm_config* cfg, int dtype, int flags, up_unipose_lstm_plan** out) {
    UP_REQUIRE(cfg && out, UP_ERR_INVALID, "unipose_lstm_plan_create: null argument");
    UP_REQUIRE(dtype == UP_DT_F32 || dtype == UP_DT_BF16, UP_ERR_INVALID,
               "unipose_lstm_plan_create: storage type %d (UP_DT_F32 or UP_DT_BF16)", dtype);
    UP_REQUIRE((flags & ~UP_PLAN_FLIP_ONE_PASS) == 0, UP_ERR_INVALID, "unipose_lstm_plan_create: flags %d (UP_PLAN_FLIP_ONE_PASS or 0)",
               flags);
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
    pl->dtype = dtype;
    pl->flags = flags;
    for (size_t f = 0; f < LSTM_FORMS; ++f) {
        const plan::Program& g = plan::LSTM_PROGRAMS[f];
        plan::build_lstm(pl->prog[f], pl->cfg, g, dtype, (flags & UP_PLAN_FLIP_ONE_PASS) != 0);
        if (g.counts == plan::COUNTS_PLAIN) pl->ws_bytes = std::max(pl->ws_bytes, pl->prog[f].ws_bytes);
        if (g.counts == plan::COUNTS_FLIP) pl->flip_ws_bytes = std::max(pl->flip_ws_bytes, pl->prog[f].ws_bytes);
        for (const plan::Op& op : pl->prog[f].ops)       // the hidden state STATE_OUT copies: its tensor's padded size
            if (op.kind == plan::STATE_OUT) pl->state_half = pl->prog[f].tensors[op.in.id].bytes / sizeof(float);
    }
    const int cg = cfg->num_classes + 2;
    const bool ok = pl->w.bind(pl->prog, LSTM_FORMS, cg);
    // the listed convolutions: the trunk in program order (wasp.conv2 twice, like the image plan), the gate parts, the head
    static const char* const gates0[3] = {"g", "i", "o"};
    static const char* const gates[8] = {"gx", "ix", "ox", "fx", "gh", "ih", "oh", "fh"};
    for (const plan::Conv& cv : pl->prog[0].convs) {
        if (cv.name == "lstm_0") {
            for (int i = 0; i < 3; ++i)
                pl->w.list(std::string("lstm_0.conv_") + gates0[i] + "_lstm", pl->w.store_of("lstm_0"), i, cg, cg, 3, true);
            for (int i = 0; i < 8; ++i)
                pl->w.list(std::string("lstm.conv_") + gates[i] + "_lstm", pl->w.store_of("lstm"), i, cg, cg, 3, true);
            continue;
        }
        pl->w.list(cv.name, pl->w.store_of(cv.name), -1, cv.d.K, cv.d.C, cv.d.R, cv.has_bias);
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
    pl->w.release();
    delete pl;
}

extern "C" int up_unipose_lstm_plan_num_convs(const up_unipose_lstm_plan* pl) { return plan::num_convs(pl ? &pl->w : nullptr); }

extern "C" const char* up_unipose_lstm_plan_conv_name(const up_unipose_lstm_plan* pl, int i) {
    return plan::conv_name(pl ? &pl->w : nullptr, i);
}

extern "C" int up_unipose_lstm_plan_conv_shape(const up_unipose_lstm_plan* pl, int i, int32_t* oihw, int32_t* has_bias) {
    return plan::conv_shape(pl ? &pl->w : nullptr, i, oihw, has_bias, "unipose_lstm_plan_conv_shape");
}

extern "C" int up_unipose_lstm_plan_set_conv(up_unipose_lstm_plan* pl, int i, const float* w_oihw, const float* bias, void* stream) {
    if (int e = plan::set_conv_check(pl ? &pl->w : nullptr, i, w_oihw, bias, "unipose_lstm_plan_set_conv")) return e;
    plan::Entry& en = pl->w.entries[i];
    if (en.part < 0) return plan::set_conv_whole(pl->w, i, w_oihw, bias, stream);
    // a gate part: rows [gate * cg, (gate + 1) * cg) of the stacked OIHW image, input channels from xoff on
    plan::Store& st = pl->w.stores[en.store];
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
    for (const plan::Entry& other : pl->w.entries)
        if (other.store == en.store && !other.set) return UP_OK;
    // every part is set: the stacked bias (LSTM_0: g | i | o; LSTM: bx + bh per gate) and the packed image
    int e = st.parts == 3 ? up_copy2d(st.stage_b, 3 * cg, st.bias, 3 * cg, 1, 3 * cg, stream)
                          : up_add2d(st.stage_b, cg, st.stage_b + 4 * cg, cg, st.bias, cg, 4, cg, stream);
    if (e) return e;
    return plan::pack(pl->w, st, st.stage_w, stream);
}

extern "C" size_t up_unipose_lstm_plan_workspace(const up_unipose_lstm_plan* pl) { return pl ? pl->ws_bytes : 0; }

extern "C" size_t up_unipose_lstm_plan_flip_workspace(const up_unipose_lstm_plan* pl) { return pl ? pl->flip_ws_bytes : 0; }

extern "C" size_t up_unipose_lstm_plan_program_workspace(const up_unipose_lstm_plan* pl, int program) {
    return pl ? plan::program_workspace(plan::LSTM_PROGRAMS, pl->prog, program) : 0;
}

extern "C" size_t up_unipose_lstm_plan_state_bytes(const up_unipose_lstm_plan* pl) {
    return pl ? 2 * pl->state_half * sizeof(float) : 0;
}

// one record of a state pool in floats: hide then cell, (h, w, rup4(K + 2)) each, the stride rounded up to 256 bytes
static size_t pool_record(const up_unipose_lstm_plan* pl) {
    const size_t h = (pl->cfg.height - 1) / 8 + 1, w = (pl->cfg.width - 1) / 8 + 1, ldo = plan::rup4(pl->cfg.num_classes + 2);
    return (2 * h * w * ldo + 63) / 64 * 64;
}

extern "C" size_t up_unipose_lstm_plan_pool_bytes(const up_unipose_lstm_plan* pl, int slots) {
    return pl && slots >= 1 ? (size_t)slots * pool_record(pl) * sizeof(float) : 0;
}

// The program of an entry's arguments, ready and run: a too-small workspace is UP_ERR_WORKSPACE from this plan.  whole: step and clip
// ask for up_unipose_lstm_plan_workspace() (as ever), the evaluation entries for their program's own need.
static int launch(up_unipose_lstm_plan* pl, plan::Input input, bool flip, plan::Ending end, plan::State from, bool whole, const plan::Io& io,
                  void* workspace, size_t ws_bytes, void* stream, const char* what) {
    const Plan& prog = pl->prog[plan::find(plan::LSTM_PROGRAMS, input, flip, end, from)];
    return plan::launch(pl->w, "up_unipose_lstm_plan_set_conv", prog, whole ? pl->ws_bytes : prog.ws_bytes, UP_ERR_WORKSPACE, io, workspace,
                        ws_bytes, stream, what);
}

extern "C" int up_unipose_lstm_step(up_unipose_lstm_plan* pl, const float* x_nchw, const float* center_nchw, const float* prev_hide,
                                    const float* prev_cell, float* heat_nchw, float* cell_nchw, float* hide_nchw, void* workspace,
                                    size_t ws_bytes, void* stream) {
    UP_REQUIRE(pl && x_nchw && center_nchw && heat_nchw && cell_nchw && hide_nchw && workspace, UP_ERR_INVALID,
               "unipose_lstm_step: null argument");
    UP_REQUIRE((prev_hide == nullptr) == (prev_cell == nullptr), UP_ERR_INVALID,
               "unipose_lstm_step: prev_hide and prev_cell are both given (a later frame) or both NULL (the first frame)");
    plan::Io io;
    io.x = x_nchw;
    io.center = center_nchw;
    io.prev_hide = prev_hide;
    io.prev_cell = prev_cell;
    io.heat = heat_nchw;
    io.cell = cell_nchw;
    io.hide = hide_nchw;
    return launch(pl, plan::IN_NCHW, false, plan::END_HEAT, prev_hide ? plan::STATE_NCHW : plan::STATE_NONE, true, io, workspace, ws_bytes,
                  stream, "unipose_lstm_step");
}

extern "C" int up_unipose_lstm_clip(up_unipose_lstm_plan* pl, const float* x, const float* center, float* heat, float* cell_last,
                                    float* hide_last, void* workspace, size_t ws_bytes, void* stream) {
    UP_REQUIRE(pl && x && center && heat && workspace, UP_ERR_INVALID, "unipose_lstm_clip: null argument");
    plan::Io io;
    io.x = x;
    io.center = center;
    io.heat = heat;
    io.cell = cell_last;
    io.hide = hide_last;
    return launch(pl, plan::IN_CLIP, false, plan::END_HEAT, plan::STATE_NONE, true, io, workspace, ws_bytes, stream, "unipose_lstm_clip");
}

// the evaluation entries
extern "C" int up_unipose_lstm_clip_keypoints(up_unipose_lstm_plan* pl, const float* x, const float* center, int out_h, int out_w,
                                              int32_t* idx, float* preds_xy, float* maxvals, float* cell_last, float* hide_last,
                                              void* workspace, size_t ws_bytes, void* stream) {
    UP_REQUIRE(pl && x && center && preds_xy && maxvals && workspace, UP_ERR_INVALID, "unipose_lstm_clip_keypoints: null argument");
    if (int e = plan::grid_ok(out_h, out_w, pl->cfg.height, pl->cfg.width, "unipose_lstm_clip_keypoints")) return e;
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
    return launch(pl, plan::IN_CLIP, false, plan::END_DECODE, plan::STATE_NONE, false, io, workspace, ws_bytes, stream,
                  "unipose_lstm_clip_keypoints");
}

extern "C" int up_unipose_lstm_clip_flip(up_unipose_lstm_plan* pl, const float* x, const float* center, const int32_t* perm_host,
                                         float* heat, void* workspace, size_t ws_bytes, void* stream) {
    UP_REQUIRE(pl && x && center && perm_host && heat && workspace, UP_ERR_INVALID, "unipose_lstm_clip_flip: null argument");
    if (int e = plan::perm_ok(pl->cfg.num_classes + 1, "heat-map", perm_host, "unipose_lstm_clip_flip")) return e;
    plan::Io io;
    io.x = x;
    io.center = center;
    io.perm = perm_host;
    io.heat = heat;
    return launch(pl, plan::IN_CLIP, true, plan::END_HEAT, plan::STATE_NONE, false, io, workspace, ws_bytes, stream, "unipose_lstm_clip_flip");
}

extern "C" int up_unipose_lstm_clip_final_preds(up_unipose_lstm_plan* pl, const float* x, const float* center, const int32_t* perm_host,
                                                const double* inv, int res0, int res1, float* preds_xy, float* coords_xy,
                                                float* maxvals, void* workspace, size_t ws_bytes, void* stream) {
    UP_REQUIRE(pl && x && center && preds_xy && maxvals && workspace, UP_ERR_INVALID, "unipose_lstm_clip_final_preds: null argument");
    UP_REQUIRE(res0 > 0 && res1 > 0, UP_ERR_INVALID, "unipose_lstm_clip_final_preds: res %d, %d", res0, res1);
    if (perm_host)
        if (int e = plan::perm_ok(pl->cfg.num_classes + 1, "heat-map", perm_host, "unipose_lstm_clip_final_preds")) return e;
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
    return launch(pl, plan::IN_CLIP, perm_host != nullptr, plan::END_FINAL, plan::STATE_NONE, false, io, workspace, ws_bytes, stream,
                  "unipose_lstm_clip_final_preds");
}

extern "C" int up_unipose_lstm_stream_keypoints(up_unipose_lstm_plan* pl, const float* x_nchw, const float* center_nchw, void* state,
                                                int first, int out_h, int out_w, int32_t* idx, float* preds_xy, float* maxvals,
                                                float* heat_nchw, void* workspace, size_t ws_bytes, void* stream) {
    UP_REQUIRE(pl && x_nchw && center_nchw && preds_xy && maxvals && workspace, UP_ERR_INVALID,
               "unipose_lstm_stream_keypoints: null argument");
    UP_REQUIRE(state && (reinterpret_cast<uintptr_t>(state) & 255) == 0, UP_ERR_INVALID,
               "unipose_lstm_stream_keypoints: a 256-byte aligned state buffer of up_unipose_lstm_plan_state_bytes() bytes is needed");
    if (int e = plan::grid_ok(out_h, out_w, pl->cfg.height, pl->cfg.width, "unipose_lstm_stream_keypoints")) return e;
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
    return launch(pl, plan::IN_NCHW, false, plan::END_DECODE, first ? plan::STATE_NONE : plan::STATE_BUFFER, false, io, workspace, ws_bytes,
                  stream, "unipose_lstm_stream_keypoints");
}

// From source frames: up_clip_crop_to_nhwc (a stream: up_crop_to_nhwc) and the centre pool in front of the same programs.  What the
// centre-pool kernels refuse of the caller's arguments (the sizes are the plan's) is refused here, before the crop is launched.
static int lstm_frame_io(int samples, plan::Io& io, const void* src_hwc, int src_type, int F, int Hs, int Ws, const int32_t* frame_of,
                         const int32_t* valid_hw, const double* crop_inv, float border, float mean, float stdv, const double* center_xy,
                         double sigma, const char* what) {
    if (int e = frame_io(samples, io, src_hwc, src_type, F, Hs, Ws, frame_of, valid_hw, crop_inv, border, mean, stdv, what)) return e;
    UP_REQUIRE(center_xy, UP_ERR_INVALID, "%s: null centre coordinates", what);
    UP_REQUIRE(sigma > 0, UP_ERR_INVALID, "%s: sigma %g", what, sigma);
    io.center_xy = center_xy;
    io.sigma = sigma;
    return UP_OK;
}

extern "C" int up_unipose_lstm_clip_frame_heatmaps(up_unipose_lstm_plan* pl, const void* src_hwc, int src_type, int F, int Hs, int Ws,
                                                   const int32_t* frame_of, const int32_t* valid_hw, const double* crop_inv, float border,
                                                   float mean, float stdv, const double* center_xy, double sigma,
                                                   const int32_t* perm_host, float* heat, float* cell_last, float* hide_last,
                                                   void* workspace, size_t ws_bytes, void* stream) {
    UP_REQUIRE(pl && heat && workspace, UP_ERR_INVALID, "unipose_lstm_clip_frame_heatmaps: null argument");
    UP_REQUIRE(!perm_host || (!cell_last && !hide_last), UP_ERR_INVALID,
               "unipose_lstm_clip_frame_heatmaps: the flip test returns no state (there are two): cell_last and hide_last must be NULL");
    plan::Io io;
    if (int e = lstm_frame_io(pl->cfg.batch * pl->cfg.frames, io, src_hwc, src_type, F, Hs, Ws, frame_of, valid_hw, crop_inv, border, mean,
                              stdv, center_xy, sigma, "unipose_lstm_clip_frame_heatmaps"))
        return e;
    if (perm_host)
        if (int e = plan::perm_ok(pl->cfg.num_classes + 1, "heat-map", perm_host, "unipose_lstm_clip_frame_heatmaps")) return e;
    io.perm = perm_host;
    io.heat = heat;
    io.cell = cell_last;
    io.hide = hide_last;
    return launch(pl, plan::IN_CLIP_FRAMES, perm_host != nullptr, plan::END_HEAT, plan::STATE_NONE, false, io, workspace, ws_bytes, stream,
                  "unipose_lstm_clip_frame_heatmaps");
}

extern "C" int up_unipose_lstm_clip_frame_final_preds(up_unipose_lstm_plan* pl, const void* src_hwc, int src_type, int F, int Hs, int Ws,
                                                      const int32_t* frame_of, const int32_t* valid_hw, const double* crop_inv,
                                                      float border, float mean, float stdv, const double* center_xy, double sigma,
                                                      const int32_t* perm_host, const double* inv, int res0, int res1, float* preds_xy,
                                                      float* coords_xy, float* maxvals, void* workspace, size_t ws_bytes, void* stream) {
    UP_REQUIRE(pl && preds_xy && maxvals && workspace, UP_ERR_INVALID, "unipose_lstm_clip_frame_final_preds: null argument");
    UP_REQUIRE(res0 > 0 && res1 > 0, UP_ERR_INVALID, "unipose_lstm_clip_frame_final_preds: res %d, %d", res0, res1);
    plan::Io io;
    if (int e = lstm_frame_io(pl->cfg.batch * pl->cfg.frames, io, src_hwc, src_type, F, Hs, Ws, frame_of, valid_hw, crop_inv, border, mean,
                              stdv, center_xy, sigma, "unipose_lstm_clip_frame_final_preds"))
        return e;
    if (perm_host)
        if (int e = plan::perm_ok(pl->cfg.num_classes + 1, "heat-map", perm_host, "unipose_lstm_clip_frame_final_preds")) return e;
    io.perm = perm_host;
    io.inv = inv;
    io.res0 = res0;
    io.res1 = res1;
    io.preds = preds_xy;
    io.coords = coords_xy;
    io.maxvals = maxvals;
    return launch(pl, plan::IN_CLIP_FRAMES, perm_host != nullptr, plan::END_FINAL, plan::STATE_NONE, false, io, workspace, ws_bytes, stream,
                  "unipose_lstm_clip_frame_final_preds");
}

extern "C" int up_unipose_lstm_stream_frame_final_preds(up_unipose_lstm_plan* pl, const void* src_hwc, int src_type, int F, int Hs, int Ws,
                                                        const int32_t* frame_of, const int32_t* valid_hw, const double* crop_inv,
                                                        float border, float mean, float stdv, const double* center_xy, double sigma,
                                                        void* state, int first, const double* inv, int res0, int res1, float* preds_xy,
                                                        float* coords_xy, float* maxvals, float* heat_nchw, void* workspace,
                                                        size_t ws_bytes, void* stream) {
    UP_REQUIRE(pl && preds_xy && maxvals && workspace, UP_ERR_INVALID, "unipose_lstm_stream_frame_final_preds: null argument");
    UP_REQUIRE(state && (reinterpret_cast<uintptr_t>(state) & 255) == 0, UP_ERR_INVALID,
               "unipose_lstm_stream_frame_final_preds: a 256-byte aligned state buffer of up_unipose_lstm_plan_state_bytes() bytes is needed");
    UP_REQUIRE(res0 > 0 && res1 > 0, UP_ERR_INVALID, "unipose_lstm_stream_frame_final_preds: res %d, %d", res0, res1);
    plan::Io io;
    if (int e = lstm_frame_io(pl->cfg.batch, io, src_hwc, src_type, F, Hs, Ws, frame_of, valid_hw, crop_inv, border, mean, stdv, center_xy,
                              sigma, "unipose_lstm_stream_frame_final_preds"))
        return e;
    io.state = static_cast<float*>(state);
    io.state_half = pl->state_half;
    io.inv = inv;
    io.res0 = res0;
    io.res1 = res1;
    io.preds = preds_xy;
    io.coords = coords_xy;
    io.maxvals = maxvals;
    io.heat = heat_nchw;
    return launch(pl, plan::IN_FRAMES, false, plan::END_FINAL, first ? plan::STATE_NONE : plan::STATE_BUFFER, false, io, workspace, ws_bytes,
                  stream, "unipose_lstm_stream_frame_final_preds");
}

// ---- many streams in one call: the state in a pool of per-stream records ----------------------------------------------------------------
// What both serving entries check of the pool and the table, before anything is launched, and the Io fields of GATHER / SERVE.
static int serve_io(up_unipose_lstm_plan* pl, plan::Io& io, void* pool, int slots, const int32_t* slot_host, const int32_t* first_host,
                    const char* what) {
    UP_REQUIRE(pl->cfg.batch <= UP_SERVE_CAP, UP_ERR_UNSUPPORTED, "%s: a plan of batch %d (the table holds up to %d samples)", what,
               pl->cfg.batch, (int)UP_SERVE_CAP);
    UP_REQUIRE(pool && (reinterpret_cast<uintptr_t>(pool) & 255) == 0, UP_ERR_INVALID,
               "%s: a 256-byte aligned pool of up_unipose_lstm_plan_pool_bytes(plan, slots) bytes is needed", what);
    if (int e = serve_table_check(what, slots, slot_host, first_host, pl->cfg.batch, &io.firsts, &io.nexts)) return e;
    io.pool = static_cast<float*>(pool);
    io.slot_stride = (int64_t)pool_record(pl);
    io.slots = slots;
    io.slot_host = slot_host;
    io.first_host = first_host;
    return UP_OK;
}

extern "C" int up_unipose_lstm_serve_keypoints(up_unipose_lstm_plan* pl, const float* x_nchw, const float* center_nchw, void* pool, int slots,
                                               const int32_t* slot_host, const int32_t* first_host, int out_h, int out_w, int32_t* idx,
                                               float* preds_xy, float* maxvals, float* heat_nchw, void* workspace, size_t ws_bytes,
                                               void* stream) {
    UP_REQUIRE(pl && x_nchw && center_nchw && preds_xy && maxvals && workspace, UP_ERR_INVALID, "unipose_lstm_serve_keypoints: null argument");
    plan::Io io;
    if (int e = serve_io(pl, io, pool, slots, slot_host, first_host, "unipose_lstm_serve_keypoints")) return e;
    if (int e = plan::grid_ok(out_h, out_w, pl->cfg.height, pl->cfg.width, "unipose_lstm_serve_keypoints")) return e;
    io.x = x_nchw;
    io.center = center_nchw;
    io.dec_h = out_h;
    io.dec_w = out_w;
    io.idx = idx;
    io.preds = preds_xy;
    io.maxvals = maxvals;
    io.heat = heat_nchw;
    return launch(pl, plan::IN_NCHW, false, plan::END_DECODE, plan::STATE_POOL, false, io, workspace, ws_bytes, stream,
                  "unipose_lstm_serve_keypoints");
}

extern "C" int up_unipose_lstm_serve_frame_final_preds(up_unipose_lstm_plan* pl, const void* src_hwc, int src_type, int F, int Hs, int Ws,
                                                       const int32_t* frame_of, const int32_t* valid_hw, const double* crop_inv,
                                                       float border, float mean, float stdv, const double* center_xy, double sigma,
                                                       void* pool, int slots, const int32_t* slot_host, const int32_t* first_host,
                                                       const double* inv, int res0, int res1, float* preds_xy, float* coords_xy,
                                                       float* maxvals, float* heat_nchw, void* workspace, size_t ws_bytes, void* stream) {
    UP_REQUIRE(pl && preds_xy && maxvals && workspace, UP_ERR_INVALID, "unipose_lstm_serve_frame_final_preds: null argument");
    UP_REQUIRE(res0 > 0 && res1 > 0, UP_ERR_INVALID, "unipose_lstm_serve_frame_final_preds: res %d, %d", res0, res1);
    plan::Io io;
    if (int e = serve_io(pl, io, pool, slots, slot_host, first_host, "unipose_lstm_serve_frame_final_preds")) return e;
    if (int e = lstm_frame_io(pl->cfg.batch, io, src_hwc, src_type, F, Hs, Ws, frame_of, valid_hw, crop_inv, border, mean, stdv, center_xy,
                              sigma, "unipose_lstm_serve_frame_final_preds"))
        return e;
    io.inv = inv;
    io.res0 = res0;
    io.res1 = res1;
    io.preds = preds_xy;
    io.coords = coords_xy;
    io.maxvals = maxvals;
    io.heat = heat_nchw;
    return launch(pl, plan::IN_FRAMES, false, plan::END_FINAL, plan::STATE_POOL, false, io, workspace, ws_bytes, stream,
                  "unipose_lstm_serve_frame_final_preds");
}
