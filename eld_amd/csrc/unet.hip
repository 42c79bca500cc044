// unet.hip -- host-side orchestration of the SID U-Net forward / backward over the HIP kernels, and
// the C-ABI entry points of include/eld_amd.h for it.  No allocation, no synchronisation: every launch
// goes to the caller's stream and all scratch comes out of the caller's workspace, so a whole training
// step is one stream-ordered chain (hipGraph-capturable).
//
// Network (models/arch/Unet.py:6-91): 5 scales, channels 32/64/128/256/512, 18 conv3x3+LeakyReLU,
// 4 maxpool2, 4 transposed conv 2x2/s2, 4 channel concats [up, skip] (never materialised: the conv
// kernels read two sources), 1x1 head.
#include <mutex>
#include <unordered_map>
#include <math.h>
#include "unet_misc.h"

namespace {

constexpr int NLEV = 5;
inline int chan(int l) { return 32 << l; }

struct LayerDef {
    int kind;        // 0 conv3x3, 1 convT2x2, 2 head 1x1
    int cin, cout;
    size_t w_off, b_off;      // flat parameter offsets (floats)
};

// layer order == named_parameters() order of the reference module
enum {
    L_E0A = 0, L_E0B, L_E1A, L_E1B, L_E2A, L_E2B, L_E3A, L_E3B, L_E4A, L_E4B,
    L_UP3, L_D3A, L_D3B, L_UP2, L_D2A, L_D2B, L_UP1, L_D1A, L_D1B, L_UP0, L_D0A, L_D0B, L_HEAD, NLAYERS
};
// resolution level of layer i's OUTPUT (a transposed conv reads level + 1)
inline int layer_level(int i) { return i <= L_E4B ? i / 2 : (i < L_HEAD ? 3 - (i - L_UP3) / 3 : 0); }

size_t build_layers(int in_ch, int out_ch, LayerDef* L) {
    int k = 0;
    for (int l = 0; l < NLEV; ++l) {
        L[k++] = {0, l == 0 ? in_ch : chan(l - 1), chan(l), 0, 0};
        L[k++] = {0, chan(l), chan(l), 0, 0};
    }
    for (int l = 3; l >= 0; --l) {
        L[k++] = {1, chan(l + 1), chan(l), 0, 0};
        L[k++] = {0, 2 * chan(l), chan(l), 0, 0};
        L[k++] = {0, chan(l), chan(l), 0, 0};
    }
    L[k++] = {2, 32, out_ch, 0, 0};
    size_t off = 0;
    for (int i = 0; i < NLAYERS; ++i) {
        const size_t taps = L[i].kind == 0 ? 9 : (L[i].kind == 1 ? 4 : 1);
        L[i].w_off = off; off += (size_t)L[i].cin * L[i].cout * taps;
        L[i].b_off = off; off += L[i].cout;
    }
    return off;
}

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

int choose_psplit(int groups, int ntiles) {
    int ps = 512 / groups;
    if (ps < 1) ps = 1;
    if (ps > ntiles) ps = ntiles;
    if (ps < 1) ps = 1;
    return ps;
}

struct WgradGeom { int T, CA, CBp, groups, ntiles, psplit, w8; size_t floats; };

// algo: the fp32 product scheme of the call (the three-piece scheme re-blocks 3x3 layers for wgrad8_kernel: one 8-wave workgroup per CU)
WgradGeom wgrad_geom(int mode, int CA, int CB, int N, int H, int W, int algo) {
    WgradGeom g;
    g.T = mode == CONV_3X3 ? 9 : 4;
    g.CA = CA;
    g.CBp = (CB + 31) / 32 * 32;
    g.w8 = 0;
    int cob8, jb8, th8, tw8;
    // algo 3 = bf16 tensors on the same re-blocked kernel (one plane per operand, 256-pixel tiles)
    if ((algo == 1 || algo == 3) && mode == CONV_3X3 && CB % 32 == 0 && wgrad8_shape(CA, g.CBp, cob8, jb8, th8, tw8, algo == 3)) {
        g.w8 = 1;
        g.groups = (CA / cob8) * (g.CBp / jb8);
        g.ntiles = wgrad8_ntiles(CA, g.CBp, N, H, W, algo == 3);
        int ps = 256 / g.groups;
        if (ps > g.ntiles) ps = g.ntiles;
        g.psplit = ps < 1 ? 1 : ps;
        g.floats = (size_t)g.psplit * ((size_t)g.T * CA * g.CBp + CA);
        return g;
    }
    // algo 1, transposed convs with >= 128 x 64 channels: wgradt8_kernel (one 8-wave workgroup per CU, 128 x 64 blocks, 8 x 8-pixel tiles per image)
    if (algo == 1 && mode == CONV_GATHER2X2 && CB == g.CBp && wgradt8_takes(CA, CB)) {
        g.w8 = 1;
        g.groups = (CA / 128) * (g.CBp / 64);
        g.ntiles = wgradt8_ntiles(N, H, W);
        int ps = 256 / g.groups;
        if (ps > g.ntiles) ps = g.ntiles;
        g.psplit = ps < 1 ? 1 : ps;
        g.floats = (size_t)g.psplit * ((size_t)g.T * CA * g.CBp + CA);
        return g;
    }
    const int COB = (CA % 64 == 0) ? 64 : 32;
    const int TH = mode == CONV_3X3 ? 4 : 2;
    g.groups = (CA / COB) * (g.CBp / 32);
    g.ntiles = ((W + 31) / 32) * ((H + TH - 1) / TH) * N;
    g.psplit = choose_psplit(g.groups, g.ntiles);
    g.floats = (size_t)g.psplit * ((size_t)g.T * CA * g.CBp + CA);
    return g;
}

// partials of one weight gradient, whichever scheme the call turns out to run (0, 1: fp32; 3: bf16, which re-blocks 3x3 layers only)
size_t wgrad_floats_max(int mode, int CA, int CB, int N, int H, int W) {
    size_t f = 0;
    for (int algo : {0, 1, 3}) { const size_t q = wgrad_geom(mode, CA, CB, N, H, W, algo).floats; f = q > f ? q : f; }
    return f;
}

// ------------------------------------------------------------------------------------------------
// layer helpers on packed weights
// ------------------------------------------------------------------------------------------------
// Operand bounds for the two-piece fp16 product scheme (conv_fp32_algo 2): set by the caller right before a helper call,
// consumed (and cleared) by it.  Slots are device floats in the workspace.
struct Amax { const float* in0 = nullptr; const float* in1 = nullptr; const float* w = nullptr; float* out0 = nullptr; float* out1 = nullptr; };
thread_local Amax g_am;
// scratch for the split-K partial sums of small problems (conv_x3.hip): the plan's weight-gradient partial region, free while a conv runs;
// set for the duration of a U-Net entry point
struct KPart { float* p = nullptr; size_t floats = 0; };
thread_local KPart g_kp;
struct KPartScope { KPart prev; KPartScope(float* p, size_t n) : prev(g_kp) { g_kp.p = p; g_kp.floats = n; } ~KPartScope() { g_kp = prev; } };
thread_local int g_algo = -1;      // fp32 product scheme of the entry point being executed on this thread (-1: process default)
struct AlgoScope { int prev; explicit AlgoScope(int a) : prev(g_algo) { g_algo = resolve_algo(a); } ~AlgoScope() { g_algo = prev; } };
inline void take_amax(ConvArgs& a) { a.algo = g_algo; a.amax_in0 = g_am.in0; a.amax_in1 = g_am.in1; a.amax_w = g_am.w; a.amax_out0 = g_am.out0; a.amax_out1 = g_am.out1; g_am = Amax(); }
inline void take_amax(WgradArgs& a) { a.algo = g_algo; a.amax_g = g_am.in0; a.amax_x0 = g_am.w; a.amax_x1 = g_am.in1; g_am = Amax(); }      // wgrad: in0 = G, w = X0, in1 = X1
enum { S_W = 0, S_X = 23, S_EA = 24, S_EB = 29, S_UP = 34, S_DA = 38, S_DB = 42, S_GA = 46, S_GB = 47, S_SKIP = 48, S_COUNT = 64 };
// The element type T of activations and packed weights (float / bf16_t) decides ConvArgs::dtype and the weight-gradient scheme wgrad_geom sizes for;
// the bf16 launchers never look at algo, kpart or the operand bounds (launch_conv / launch_wgrad branch on dtype first).
template <typename T> struct Elem;
template <> struct Elem<float> {
    static constexpr int dtype = DT_F32, bf16 = 0;
    static constexpr int x_pad = 16;                     // channels of the converted NHWC input of conv1_1 (more than 4 planes): one K granule
    static int wgrad_scheme() { return g_algo; }
    static int gather_scheme() { return g_algo == 1 ? 1 : 0; }
    static bool conv_pools(int, int, int, int) { return g_algo == 1; }      // the three-piece 3x3 kernels also write the 2x2 max-pool of their output
    static bool reads_codes() { return g_algo == 1; }                      // only the three-piece backward-data epilogues and their pool backward read codes
};
template <> struct Elem<bf16_t> {
    static constexpr int dtype = DT_BF16, bf16 = 1;
    static constexpr int x_pad = 32;
    static int wgrad_scheme() { return 3; }
    static int gather_scheme() { return 0; }
    static bool conv_pools(int C, int N, int H, int W) { return bfd_slab_bn(C, C, N, H, W) != 0; }      // C -> C layers on the DMA kernel (conv_bfd.hip) do
    static bool reads_codes() { return true; }
};

template <typename T>
int conv_fwd(const T* in0, int C0, const T* in1, int C1, const T* wp, const float* bias, T* out, int N, int H, int W,
             int Cout, int lrelu, hipStream_t st, T* pool_out = nullptr, unsigned* codes_out = nullptr, unsigned* pool_codes_out = nullptr) {
    ConvArgs a = {};
    a.pool_out = pool_out;
    a.codes_out = codes_out;
    a.pool_codes_out = pool_codes_out;
    a.in0 = in0; a.in1 = in1; a.C0 = C0; a.C1 = C1; a.wp = wp; a.N = N; a.H = H; a.W = W; a.Nout = Cout;
    a.epi = EPI_FWD; a.bias = bias; a.lrelu = lrelu; a.out0 = out; a.dtype = Elem<T>::dtype;
    a.kpart = g_kp.p; a.kpart_floats = g_kp.floats;
    take_amax(a);
    return launch_conv(a, CONV_3X3, st);
}

// g: [N,H,W,Cout] -> din (Cin channels, split over out0/out1), wb packed [9][Cin][Cout]
template <typename T>
int conv_bwd_data(const T* g, const T* wb, T* out0, T* out1, int split, const T* act0, const T* act1, int N, int H,
                  int W, int Cin, int Cout, hipStream_t st, const unsigned* codes0 = nullptr) {
    ConvArgs a = {};
    a.codes0 = codes0;
    a.in0 = g; a.C0 = Cout; a.wp = wb; a.N = N; a.H = H; a.W = W; a.Nout = Cin;
    a.epi = EPI_GRAD; a.out0 = out0; a.out1 = out1; a.split = split; a.act0 = act0; a.act1 = act1; a.dtype = Elem<T>::dtype;
    a.kpart = g_kp.p; a.kpart_floats = g_kp.floats;
    take_amax(a);
    return launch_conv(a, CONV_3X3, st);
}

// Cin_real: the weight tensor's input channels (less than C0 + C1 where x0 is zero padded beyond them: conv1_1 with more than 4 planes)
template <typename T>
int conv_wgrad(const T* g, int Cout, const T* x0, int C0, const T* x1, int C1, int Cin_real, float* dw, float* db, float* part,
               int N, int H, int W, hipStream_t st) {
    const WgradGeom q = wgrad_geom(CONV_3X3, Cout, C0 + C1, N, H, W, (C0 % 32 || C1 % 32) ? 0 : Elem<T>::wgrad_scheme());
    WgradArgs a = {};
    a.g = g; a.CA = Cout; a.x0 = x0; a.x1 = x1; a.C0 = C0; a.C1 = C1; a.N = N; a.H = H; a.W = W; a.dtype = Elem<T>::dtype;
    a.part = part; a.bpart = db ? part + (size_t)q.psplit * q.T * q.CA * q.CBp : nullptr; a.CBp = q.CBp; a.psplit = q.psplit;
    take_amax(a);
    a.wgrad8 = q.w8;
    int rc = launch_wgrad(a, CONV_3X3, st);
    if (rc) return rc;
    return launch_wgrad_reduce(part, a.bpart, dw, db, q.psplit, q.T, q.CA, q.CBp, Cin_real, st);
}

// in [N,H,W,Cin] -> out [N,2H,2W,Cout]; wf packed [4*Cout][Cin]
template <typename T>
int convt_fwd(const T* in, const T* wf, const float* bias, T* out, int N, int H, int W, int Cin, int Cout, hipStream_t st) {
    ConvArgs a = {};
    a.in0 = in; a.C0 = Cin; a.wp = wf; a.N = N; a.H = H; a.W = W; a.Nout = 4 * Cout;
    a.epi = EPI_CONVT_FWD; a.bias = bias; a.out0 = out; a.Cout_t = Cout; a.dtype = Elem<T>::dtype;
    take_amax(a);
    return launch_conv(a, CONV_1X1, st);
}

// dout [N,2H,2W,Cout] -> din [N,H,W,Cin] (times slope(act) if act); wb packed [4][Cin][Cout]
template <typename T>
int convt_bwd_data(const T* dout, const T* wb, const T* act, T* din, int N, int H, int W, int Cin, int Cout, hipStream_t st) {
    ConvArgs a = {};
    a.in0 = dout; a.C0 = Cout; a.wp = wb; a.N = N; a.H = H; a.W = W; a.Nout = Cin;
    a.epi = EPI_GRAD; a.out0 = din; a.split = Cin; a.act0 = act; a.dtype = Elem<T>::dtype;
    take_amax(a);
    return launch_conv(a, CONV_GATHER2X2, st);
}

// dw[ci][co][tap] = sum in[p][ci] * dout[gather(p,tap)][co];  db[co] = column sums of dout
template <typename T>
int convt_wgrad(const T* in, const T* dout, float* dw, float* db, float* part, int N, int H, int W, int Cin, int Cout, hipStream_t st) {
    const WgradGeom q = wgrad_geom(CONV_GATHER2X2, Cin, Cout, N, H, W, Elem<T>::gather_scheme());
    WgradArgs a = {};
    a.g = in; a.CA = Cin; a.x0 = dout; a.C0 = Cout; a.N = N; a.H = H; a.W = W; a.dtype = Elem<T>::dtype;
    a.part = part; a.bpart = nullptr; a.CBp = q.CBp; a.psplit = q.psplit; a.wgrad8 = q.w8;
    // bias gradient = column sums of dout: accumulated by the weight-gradient kernel from its staging registers (every dout pixel
    // passes through exactly once per block column); the partials take the plan's bias slot (psplit * CA floats >= psplit * CBp).
    // Every transposed conv of the network qualifies (CBp = C <= CA = 2C, C % 32 == 0); other shapes reach this through the single-layer entry points
    const bool fused_bias = db != nullptr && q.CBp <= q.CA && Cout == q.CBp;
    a.xbpart = fused_bias ? part + (size_t)q.psplit * q.T * q.CA * q.CBp : nullptr;
    take_amax(a);
    int rc = launch_wgrad(a, CONV_GATHER2X2, st);
    if (rc) return rc;
    // (the bias partials ride in the same reduction launch: one launch less per transposed conv)
    rc = launch_wgrad_reduce(part, fused_bias ? a.xbpart : nullptr, dw, fused_bias ? db : nullptr, q.psplit, q.T, q.CA, q.CBp, Cout, st, q.CBp);
    if (rc || !db || fused_bias) return rc;
    return launch_colsum(dout, db, part, (size_t)N * 4 * H * W, Cout, st);
}

// ------------------------------------------------------------------------------------------------
// workspace plan
// ------------------------------------------------------------------------------------------------
struct Plan {
    LayerDef L[NLAYERS];
    size_t nparams;
    int N, H, W, in_ch, out_ch;
    int Hl[NLEV], Wl[NLEV];
    // offsets in floats
    size_t wp_fwd[NLAYERS], wp_bwd[NLAYERS];
    size_t x16, ea[NLEV], eb[NLEV], pool[NLEV - 1], up[NLEV - 1], da[NLEV - 1], db[NLEV - 1];
    size_t gA, gB, skip[NLEV - 1], part, part_floats, amax;
    size_t head_part; // partials of the fused training head (eld_unet_forward_loss_ex -> the backward)
    // slope codes (conv.h ConvArgs::codes_out) of the activations the 32- / 64-channel backward-data epilogues multiply by: ea[0], ea[1], da[0], da[1]
    // (2 bits per element); written by the fp32 three-piece forward where `codes` is set (see make_plan) and, for ea[0] / da[0], by the bf16 forward
    // (fwd_code_mask); read by the backward for the regions the last forward reports (FusedFwd::codes)
    size_t cd_ea[2], cd_da[2];
    // round 6: slope codes of eb[0], eb[1] and argmax codes of pool[0], pool[1] (ConvArgs::pool_codes_out): what maxpool_bwd_codes_kernel reads instead of eb
    size_t cd_eb[2], pc[2];
    bool codes;
    size_t total;     // floats
};

int make_plan(Plan& P, int N, int H, int W, int in_ch, int out_ch) {
    if (N < 1 || H < 16 || W < 16 || (H % 16) || (W % 16)) return ELD_EINVAL;     // 4 pool levels (Unet.py:51-63)
    if (in_ch < 1 || in_ch > 16 || out_ch < 1 || out_ch > 16) return ELD_ENOTSUP;
    P.N = N; P.H = H; P.W = W; P.in_ch = in_ch; P.out_ch = out_ch;
    P.nparams = build_layers(in_ch, out_ch, P.L);
    for (int l = 0; l < NLEV; ++l) { P.Hl[l] = H >> l; P.Wl[l] = W >> l; }
    size_t off = 0;
    auto take = [&](size_t n) { const size_t o = off; off += align_up(n, 64); return o; };   // 256-byte aligned
    for (int i = 0; i < NLAYERS; ++i) {
        const LayerDef& d = P.L[i];
        if (d.kind == 0) {
            const int cinp = (d.cin + 15) / 16 * 16;
            P.wp_fwd[i] = take((size_t)9 * d.cout * cinp * 2);          // fp32 [tap][n][c] or the pre-split slab layout (7 B per element)
            P.wp_bwd[i] = (i == L_E0A) ? 0 : take((size_t)9 * d.cin * d.cout * 2);
        } else if (d.kind == 1) {
            P.wp_fwd[i] = take((size_t)4 * d.cout * d.cin);
            P.wp_bwd[i] = take((size_t)4 * d.cin * d.cout);
        } else {
            P.wp_fwd[i] = P.wp_bwd[i] = 0;
        }
    }
    auto act = [&](int l, int c) { return (size_t)N * P.Hl[l] * P.Wl[l] * c; };
    P.x16 = take(act(0, 16));
    for (int l = 0; l < NLEV; ++l) { P.ea[l] = take(act(l, chan(l))); P.eb[l] = take(act(l, chan(l))); }
    for (int l = 0; l < NLEV - 1; ++l) {
        P.pool[l] = take(act(l + 1, chan(l)));
        P.up[l] = take(act(l, chan(l)));
        P.da[l] = take(act(l, chan(l)));
        P.db[l] = take(act(l, chan(l)));
        P.skip[l] = take(act(l, chan(l)));
    }
    P.gA = take(act(0, 32));
    P.gB = take(act(0, 32));
    P.head_part = take(head_train_ws_floats(out_ch));       // out_ch <= 4: the sizes of the quad-lane head (unet_misc.hip), unchanged
    size_t pmax = head_bwd_ws_floats(out_ch);
    pmax = pmax > conv_first_wgrad_ws_floats() ? pmax : conv_first_wgrad_ws_floats();
    pmax = pmax > colsum_ws_floats(256) ? pmax : colsum_ws_floats(256);
    for (int i = 0; i < NLAYERS; ++i) {
        const LayerDef& d = P.L[i];
        const int lev = layer_level(i);
        size_t f = 0;
        if (d.kind == 0) f = wgrad_floats_max(CONV_3X3, d.cout, i == L_E0A ? 16 : d.cin, N, P.Hl[lev], P.Wl[lev]);
        else if (d.kind == 1) f = wgrad_floats_max(CONV_GATHER2X2, d.cin, d.cout, N, P.Hl[lev + 1], P.Wl[lev + 1]);
        pmax = f > pmax ? f : pmax;
    }
    // split-K partial sums of small problems share this region: up to 16 parts of the largest 3x3 output that can take the split
    for (int i = 0; i < NLAYERS; ++i) {
        const LayerDef& d = P.L[i];
        if (d.kind != 0) continue;
        const int lev = layer_level(i);
        const long long px8 = (long long)((P.Wl[lev] + 31) / 32) * ((P.Hl[lev] + 7) / 8) * N;
        for (int dir = 0; dir < 2; ++dir) {
            const int nout = dir ? d.cin : d.cout, k = dir ? d.cout : d.cin;
            if (nout % 64 || k % 32) continue;
            long long ks = eld_num_cus() / (px8 * (nout / 64));
            if (ks > k / 32) ks = k / 32;
            if (ks > 16) ks = 16;
            if (ks >= 2) { const size_t f = (size_t)ks * N * P.Hl[lev] * P.Wl[lev] * nout; pmax = f > pmax ? f : pmax; }
        }
    }
    P.part = take(pmax);
    P.part_floats = pmax;
    // Slope codes only where the 64-channel level-1 layers run the unsplit 8-wave kernel (conv_x3.hip x3_slab_bn: every CU gets a 16-row tile): the
    // split-K finish kernel of small problems does not write them.  Which regions a forward actually filled travels to the backward through the
    // workspace's CodesState (the fp32 scheme, the first layer's kernel and the debug mask are per-call choices).
    P.codes = conv_tile_count(N, P.Hl[1], P.Wl[1], 16, false) >= eld_num_cus();
    for (int l = 0; l < 2; ++l) {
        P.cd_ea[l] = take(act(l, chan(l)) / 16 + 64);
        P.cd_da[l] = take(act(l, chan(l)) / 16 + 64);
        P.cd_eb[l] = take(act(l, chan(l)) / 16 + 64);
        P.pc[l] = take(act(l + 1, chan(l)) / 16 + 64);
    }
    P.amax = take(S_COUNT);
    P.total = off;
    return 0;
}

// dir: PACK_FWD / PACK_BWD = the layouts one direction reads; PACK_BOTH = both in ONE launch (the fused training forward: the backward that follows
// with dout == NULL then skips its own pack launch -- the parameters it differentiates are by construction the ones the forward ran with)
enum { PACK_FWD = 0, PACK_BWD = 1, PACK_BOTH = 2 };
int pack_weights(const Plan& P, const float* params, float* ws, int dir, hipStream_t st, bool bf16 = false, float* amax = nullptr) {
    PackJobs jobs;
    jobs.n = 0;
    for (int pass = 0; pass < 2; ++pass) {
    const bool for_backward = pass == 1;
    if ((dir == PACK_FWD && for_backward) || (dir == PACK_BWD && !for_backward)) continue;
    for (int i = 0; i < NLAYERS; ++i) {
        const LayerDef& d = P.L[i];
        PackJob J = {};
        J.src_off = d.w_off; J.Cout = d.cout; J.Cin = d.cin; J.Cinp = d.cin;
        if (d.kind == 0) {
            J.T = 9;
            if (!for_backward) {
                J.kind = PACK_CONV_FWD; J.Cinp = (d.cin + 15) / 16 * 16; J.dst_off = P.wp_fwd[i];
                if (bf16 && i == L_E0A) {
                    if (d.cin <= 4) continue;        // conv_first.hip reads the fp32 weights directly
                    J.Cinp = 32;                     // more planes: the generic bf16 conv on the zero-padded NHWC32 input (bf16 K granule: 32 channels)
                }
            }
            else if (i != L_E0A) { J.kind = PACK_CONV_BWD; J.dst_off = P.wp_bwd[i]; }
            else continue;
        } else if (d.kind == 1) {
            J.T = 4;
            J.kind = for_backward ? PACK_CONVT_BWD : PACK_CONVT_FWD;
            J.dst_off = for_backward ? P.wp_bwd[i] : P.wp_fwd[i];
        } else {
            continue;
        }
        J.bf16 = bf16 ? 1 : 0;
        J.amax_slot = S_W + i;
        // three-piece scheme: 3x3 layers with GEMM N % 64 == 0 get pre-split slabs (N = Cout forward, Cin backward-data)
        const int lev = layer_level(i);            // (the layer's tile domain decides the slab's channel-block width)
        J.x3bn = (!bf16 && g_algo == 1 && d.kind == 0) ? x3_slab_bn(for_backward ? d.cin : d.cout, P.N, P.Hl[lev], P.Wl[lev]) : 0;
        // bf16: 3x3 layers the DMA kernel takes get its slab layout (GEMM N = Cout forward / Cin backward-data, K the other one)
        J.bfdbn = (bf16 && d.kind == 0) ? (for_backward ? bfd_slab_bn(d.cin, d.cout, P.N, P.Hl[lev], P.Wl[lev]) : bfd_slab_bn(d.cout, J.Cinp, P.N, P.Hl[lev], P.Wl[lev])) : 0;
        // bf16 transposed convs on conv_bfg_kernel take its slab layout (forward: GEMM N = 4 Cout, K = Cin on the input-resolution domain of level lev+1;
        // backward-data: N = Cin, K = 4 Cout)
        J.bfgbn = (bf16 && d.kind == 1) ? (for_backward ? bfg_slab_bn(true, d.cin, d.cout, 0, P.N, P.Hl[lev + 1], P.Wl[lev + 1])
                                                        : bfg_slab_bn(false, 4 * d.cout, d.cin, d.cout, P.N, P.Hl[lev + 1], P.Wl[lev + 1])) : 0;
        jobs.job[jobs.n++] = J;
    }
    }
    return launch_pack_all(jobs, params, ws, st, amax);
}

#define RC(x) do { int rc__ = (x); if (rc__) return rc__; } while (0)

// Gradient buckets for the data-parallel exchange: the backward produces parameter gradients in DESCENDING flat-buffer order
// (head, decoder level 0 .. 3, encoder level 4 .. 0 -- the reverse of named_parameters()), so once layer i's weight/bias
// gradients are enqueued every gradient at offset >= L[i].w_off is final.  done(i) records the events of all buckets that
// start at or above that offset; the caller's communication stream waits on them and all-reduces bucket by bucket while the
// rest of the backward runs.
struct BucketMarks {
    const int64_t* start = nullptr;     // ascending parameter offsets (floats)
    void* const* event = nullptr;       // hipEvent_t per bucket
    int n = 0, next = 0;                // buckets [next .. n) counted from the TOP are not recorded yet
    int done(const Plan& P, int layer, hipStream_t st) {
        while (n - 1 - next >= 0 && start[n - 1 - next] >= (int64_t)P.L[layer].w_off) {
            hipError_t e = hipEventRecord((hipEvent_t)event[n - 1 - next], st);
            if (e != hipSuccess) return (int)e;
            ++next;
        }
        return 0;
    }
};

// hl != null: the training step's fused head (output + loss + head backward), see launch_head_train
struct HeadLoss { const float* target; float* loss; int mse; float grad_scale; };

// What eld_unet_forward_loss_ex leaves for the backward that follows it with dout == NULL (besides the head's partials): both pack directions done, and
// -- when the first layer reads the NCHW input directly -- the caller's input tensor itself instead of a copy in the workspace (8 frames: 388 MB, 0.13 ms).
struct FusedFwd { bool packed = false; const float* x = nullptr; unsigned codes = 0; };
// FusedFwd::codes / the forwards' have_out: which slope-code regions the LAST forward on this workspace filled (it decides per launch: kernel choice,
// fp32 scheme, debug mask) -- the backward reads a region only when its bit is set, whatever its own switches say
enum { CODES_EA0 = 1, CODES_EA1 = 2, CODES_DA0 = 4, CODES_DA1 = 8, CODES_EB0 = 16, CODES_EB1 = 32, CODES_INFER = 256 };      // CODES_EBl: slope codes of eb[l] AND argmax codes of pool[l]      // CODES_INFER: the forward was eld_unet_infer_ex -- nothing for a backward

static_assert(CODES_EA0 == ELD_CODES_EA0 && CODES_EA1 == ELD_CODES_EA1 && CODES_DA0 == ELD_CODES_DA0 && CODES_DA1 == ELD_CODES_DA1 && CODES_EB0 == ELD_CODES_EB0 &&
              CODES_EB1 == ELD_CODES_EB1 && CODES_INFER == ELD_CODES_INFER, "eld_debug_unet_codes publishes these bits (include/eld_amd.h)");

static_assert(CODES_EA1 == CODES_EA0 << 1 && CODES_DA1 == CODES_DA0 << 1 && CODES_EB1 == CODES_EB0 << 1, "code_regions shifts the level-0 bit by the level");

// Where the regions named by a CODES_* mask lie (null: not in the mask).  The forward passes them to the launches that fill them, the backward to
// the ones that read them instead of the saved activation; the walkers themselves never look at the mask.
struct CodeRegions { unsigned *ea[NLEV] = {}, *da[NLEV] = {}, *eb[NLEV] = {}, *pc[NLEV] = {}; };
CodeRegions code_regions(const Plan& P, float* ws, unsigned mask) {
    CodeRegions r;
    auto at = [&](size_t off, unsigned bit) { return (mask & bit) ? reinterpret_cast<unsigned*>(ws + off) : nullptr; };
    for (int l = 0; l < 2; ++l) {
        r.ea[l] = at(P.cd_ea[l], CODES_EA0 << l);
        r.da[l] = at(P.cd_da[l], CODES_DA0 << l);
        r.eb[l] = at(P.cd_eb[l], CODES_EB0 << l);
        r.pc[l] = at(P.pc[l], CODES_EB0 << l);
    }
    return r;
}

// Which regions a forward fills: a per-call choice of each precision's kernels
template <typename T> unsigned fwd_code_mask(const Plan& P, bool infer);
template <> unsigned fwd_code_mask<float>(const Plan& P, bool infer) {
    // slope codes for the backward-data epilogues of levels 0 / 1 (Plan::codes), written by the three-piece kernels
    if (infer || !P.codes || g_algo != 1 || (debug_kernel_mask(-1) & 128)) return 0;
    unsigned m = CODES_EA1 | CODES_DA0 | CODES_DA1;
    if (P.in_ch > 4 || conv_first_writes_codes(P.in_ch)) m |= CODES_EA0;
    // argmax codes of the two full-size pools (bit 8 of the mask: A/B and bit-identity switch): the pool's backward then reads codes instead of eb[l].
    // Level 0: conv_x3w_kernel writes them, conv_x3_kernel<32, 4> does not
    if (!(debug_kernel_mask(-1) & 256)) m |= CODES_EB1 | (x3w_enabled() ? CODES_EB0 : 0u);
    return m;
}
template <> unsigned fwd_code_mask<bf16_t>(const Plan& P, bool infer) {
    // Slope codes of the two full-resolution activations whose backward-data epilogues run on conv_bfs_kernel (conv9_2's and conv1_2's: HBM-bound
    // launches that would otherwise re-read the saved 32-channel tensor): written by conv1_1's and conv9_1's epilogues where those kernels are the
    // ones that run (conv_first's MFMA kernel; conv_bfs for the 64 -> 32 layer) -- 8 bytes per pixel instead of 64 in the backward
    if (infer || !bfs_takes(32, 32, P.N, P.H, P.W) || (debug_kernel_mask(-1) & 128)) return 0;
    return (P.in_ch <= 4 && conv_first_writes_codes(P.in_ch) ? CODES_EA0 : 0u) | (bfs_takes(32, 64, P.N, P.H, P.W) ? CODES_DA0 : 0u);
}

// Operand bounds of the two-piece fp16 scheme along the network (Amax above): one device float per tensor (S_*) in the workspace.
// am == nullptr unless the pass is fp32 with g_algo == 2: every member then does nothing.
struct Bounds {
    float* am;
    hipStream_t st;
    void conv(int in0, int in1, int w, int out0) const {
        if (am) { g_am.in0 = am + in0; g_am.in1 = in1 >= 0 ? am + in1 : nullptr; g_am.w = am + w; g_am.out0 = am + out0; }
    }
    void wgrad(int g, int x0, int x1) const { if (am) { g_am.in0 = am + g; g_am.w = am + x0; g_am.in1 = x1 >= 0 ? am + x1 : nullptr; } }
    void bwd_data(int g, int w, int o0, int o1) const { if (am) { g_am.in0 = am + g; g_am.w = am + w; g_am.out0 = am + o0; g_am.out1 = o1 >= 0 ? am + o1 : nullptr; } }
    int clear(int slot, int n = 1) const {                           // zero slots before their tensors are (re)written
        return !am || hipMemsetAsync(am + slot, 0, n * sizeof(float), st) == hipSuccess ? 0 : (int)hipGetLastError();
    }
    int measure(const float* t, size_t n, int slot) const { return am ? launch_absmax(t, n, am + slot, st) : 0; }
    int measure(const bf16_t*, size_t, int) const { return 0; }
};
template <typename T> Bounds bounds(const Plan& P, float* ws, hipStream_t st) { return {!Elem<T>::bf16 && g_algo == 2 ? ws + P.amax : nullptr, st}; }

// T = bf16_t: bf16 activations and packed weights, fp32 accumulation / bias; the first layer reads the fp32 NCHW planes and the head writes fp32
// NCHW.  The plan's buffers are then half filled.
template <typename T>
int unet_forward(const Plan& P, const float* x, const float* prm, float* out, float* ws, hipStream_t st, const HeadLoss* hl = nullptr, unsigned* have_out = nullptr,
                 bool infer = false) {
    using E = Elem<T>;
    const int N = P.N;
    KPartScope kp(ws + P.part, P.part_floats);
    const Bounds bd = bounds<T>(P, ws, st);
    auto B = [&](size_t off) { return reinterpret_cast<T*>(ws + off); };
    RC(bd.clear(0, S_COUNT));
    RC(pack_weights(P, prm, ws, hl ? PACK_BOTH : PACK_FWD, st, E::bf16, bd.am));
    const bool first_direct = P.in_ch <= 4;        // conv1_1 straight from the NCHW planes (conv_first.hip); more planes: zero-padded NHWC in ws + P.x16
    const unsigned have = fwd_code_mask<T>(P, infer);
    const CodeRegions cd = code_regions(P, ws, have);
    if (have_out) *have_out = have;
    if (!first_direct) {      // (64 B per pixel in either precision; the backward's weight gradient reads it there)
        RC(launch_nchw_to_nhwc_pad(x, B(P.x16), N, P.in_ch, P.H, P.W, st));
    } else if (!hl && !infer) {
        // keep the input for the backward's weight gradient (the backward entry point does not receive x).  The fused training forward leaves it
        // with the caller (include/eld_amd.h: it must stay valid and unchanged until that call); inference: no backward follows
        hipError_t e = hipMemcpyAsync(ws + P.x16, x, (size_t)N * P.in_ch * P.H * P.W * sizeof(float), hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) return (int)e;
    }
    for (int l = 0; l < NLEV; ++l) {
        const LayerDef& A = P.L[2 * l]; const LayerDef& Bd = P.L[2 * l + 1];
        if (l == 0 && first_direct) {
            RC(launch_conv_first_fwd(x, prm + A.w_off, prm + A.b_off, B(P.ea[0]), N, P.in_ch, P.H, P.W, 1, st, cd.ea[0]));
            RC(bd.measure(B(P.ea[0]), (size_t)N * P.H * P.W * chan(0), S_EA));
        } else {
            if (l == 0) RC(bd.measure(B(P.x16), (size_t)N * P.H * P.W * E::x_pad, S_X));
            bd.conv(l == 0 ? S_X : S_EB + l - 1, -1, S_W + 2 * l, S_EA + l);          // pooled input is bounded by its source's bound
            RC(conv_fwd<T>(l == 0 ? B(P.x16) : B(P.pool[l - 1]), l == 0 ? E::x_pad : chan(l - 1), nullptr, 0, B(P.wp_fwd[2 * l]), prm + A.b_off, B(P.ea[l]),
                           N, P.Hl[l], P.Wl[l], chan(l), 1, st, nullptr, cd.ea[l]));
        }
        bd.conv(S_EA + l, -1, S_W + 2 * l + 1, S_EB + l);
        const bool fuse_pool = l < NLEV - 1 && E::conv_pools(chan(l), N, P.Hl[l], P.Wl[l]);      // no second pass over eb[l]
        RC(conv_fwd<T>(B(P.ea[l]), chan(l), nullptr, 0, B(P.wp_fwd[2 * l + 1]), prm + Bd.b_off, B(P.eb[l]), N, P.Hl[l], P.Wl[l], chan(l), 1, st,
                       fuse_pool ? B(P.pool[l]) : nullptr, cd.eb[l], cd.pc[l]));
        if (l < NLEV - 1 && !fuse_pool) RC(launch_maxpool_fwd(B(P.eb[l]), B(P.pool[l]), N, P.Hl[l + 1], P.Wl[l + 1], chan(l), st));
    }
    for (int l = 3; l >= 0; --l) {
        const int iu = L_UP3 + 3 * (3 - l);
        const T* src = l == 3 ? B(P.eb[4]) : B(P.db[l + 1]);
        bd.conv(l == 3 ? S_EB + 4 : S_DB + l + 1, -1, S_W + iu, S_UP + l);
        RC(convt_fwd<T>(src, B(P.wp_fwd[iu]), prm + P.L[iu].b_off, B(P.up[l]), N, P.Hl[l + 1], P.Wl[l + 1], chan(l + 1), chan(l), st));
        bd.conv(S_UP + l, S_EB + l, S_W + iu + 1, S_DA + l);
        RC(conv_fwd<T>(B(P.up[l]), chan(l), B(P.eb[l]), chan(l), B(P.wp_fwd[iu + 1]), prm + P.L[iu + 1].b_off, B(P.da[l]), N, P.Hl[l], P.Wl[l], chan(l), 1, st, nullptr,
                       cd.da[l]));
        bd.conv(S_DA + l, -1, S_W + iu + 2, S_DB + l);
        RC(conv_fwd<T>(B(P.da[l]), chan(l), nullptr, 0, B(P.wp_fwd[iu + 2]), prm + P.L[iu + 2].b_off, B(P.db[l]), N, P.Hl[l], P.Wl[l], chan(l), 1, st));
    }
    const LayerDef& Hd = P.L[L_HEAD];
    if (hl)      // training step: output, loss, the head's backward and the gradient of conv9_2's output (-> gA) in one pass
        return launch_head_train(B(P.db[0]), E::bf16, prm + Hd.w_off, prm + Hd.b_off, hl->target, out, B(P.gA), ws + P.head_part, hl->loss, N, P.H, P.W, P.out_ch,
                                 hl->mse, hl->grad_scale, st);
    return launch_head_fwd(B(P.db[0]), prm + Hd.w_off, prm + Hd.b_off, out, N, P.H, P.W, P.out_ch, st);
}

// The debug tap on the backward's activation gradients (include/eld_amd.h eld_debug_unet_grad_tap): the stage numbering, each tensor's place in the
// tap buffer, and the copy itself.  buf == nullptr (always, outside the tests): one branch per stage on the host, nothing enqueued.
enum { TAP_G_HEAD = 0, TAP_DEC = 1, TAP_ENC = 17 };       // decoder level l: TAP_DEC + 4l + {d_da, d_up, skip, d_src}; encoder level l: TAP_ENC + 3(4-l) + {d_ea, d_pool, d_eb}
static_assert(TAP_ENC + 3 * 4 + 1 == ELD_TAP_NSTAGES, "30 tapped tensors");
// stage -> channels and level of its tensor; false for a stage outside [0, ELD_TAP_NSTAGES)
bool tap_stage_shape(int stage, int& ch, int& lev) {
    if (stage < 0 || stage >= ELD_TAP_NSTAGES) return false;
    if (stage == TAP_G_HEAD) { ch = chan(0); lev = 0; return true; }
    if (stage < TAP_ENC) {
        const int l = (stage - TAP_DEC) / 4, k = (stage - TAP_DEC) % 4;
        lev = k == 3 ? l + 1 : l; ch = chan(lev);
        return true;
    }
    const int l = 4 - (stage - TAP_ENC) / 3, k = (stage - TAP_ENC) % 3;
    if (k == 0) { lev = l; ch = chan(l); }                  // d_ea[l]
    else if (k == 1) { lev = l; ch = chan(l - 1); }         // d_pool[l-1]: level l, channels of level l - 1
    else { lev = l - 1; ch = chan(l - 1); }                 // d_eb[l-1]
    return true;
}
struct GradTap {
    char* buf = nullptr;
    size_t off[ELD_TAP_NSTAGES], bytes[ELD_TAP_NSTAGES], total = 0;
    void plan(const Plan& P, int precision) {
        size_t o = 0;
        for (int s = 0; s < ELD_TAP_NSTAGES; ++s) {
            int ch = 0, lev = 0;
            tap_stage_shape(s, ch, lev);
            off[s] = o;
            bytes[s] = (size_t)P.N * P.Hl[lev] * P.Wl[lev] * ch * (precision == 1 ? 2 : 4);
            o += align_up(bytes[s], 256);
        }
        total = o;
    }
    int copy(int stage, const void* src, hipStream_t st) const {
        if (!buf) return 0;
        const hipError_t e = hipMemcpyAsync(buf + off[stage], src, bytes[stage], hipMemcpyDeviceToDevice, st);
        return e == hipSuccess ? 0 : (int)e;
    }
};

// The ping-pong buffer the backward ends in: conv1_1's weight gradient reads it, eld_debug_unet_region publishes it, unet_backward checks it at that read
constexpr size_t Plan::* GRAD_CONV1_1 = &Plan::gB;

// T = bf16_t: activation gradients bf16 (igemm on v_mfma_f32_32x32x16_bf16), weight gradients accumulated and written in fp32 (the wgrad kernels
// convert the bf16 operands while staging).
template <typename T>
int unet_backward(const Plan& P, const float* dout, const float* prm, float* grd, float* ws, hipStream_t st, BucketMarks& marks, const FusedFwd& fused, const GradTap& tap) {
    using E = Elem<T>;
    const int N = P.N;
    KPartScope kp(ws + P.part, P.part_floats);
    const Bounds bd = bounds<T>(P, ws, st);
    auto B = [&](size_t off) { return reinterpret_cast<T*>(ws + off); };
    RC(bd.clear(S_GA, S_COUNT - S_GA));
    if (!fused.packed) RC(pack_weights(P, prm, ws, PACK_BWD, st, E::bf16, bd.am));
    T* cur = B(P.gA); T* oth = B(P.gB); float* part = ws + P.part;
    auto swap = [&]() { T* t = cur; cur = oth; oth = t; };
    auto gs = [&](const T* buf) { return buf == B(P.gA) ? (int)S_GA : (int)S_GB; };               // bound slot of a ping-pong gradient buffer
    // slope codes the forward left for levels 0 / 1 (FusedFwd::codes names the regions it filled)
    const CodeRegions cd = code_regions(P, ws, E::reads_codes() ? fused.codes : 0u);
    const LayerDef& Hd = P.L[L_HEAD];
    // head: g (pre-activation grad of conv9_2) -> gA
    if (dout) RC(launch_head_bwd(dout, B(P.db[0]), prm + Hd.w_off, cur, grd + Hd.w_off, grd + Hd.b_off, part, N, P.H, P.W, P.out_ch, st));
    else RC(launch_head_train_reduce(ws + P.head_part, grd + Hd.w_off, grd + Hd.b_off, N, P.H, P.W, P.out_ch, E::bf16, st));      // gA and the partials: eld_unet_forward_loss_ex
    RC(marks.done(P, L_HEAD, st));
    RC(bd.measure(cur, (size_t)N * P.H * P.W * 32, S_GA));
    RC(tap.copy(TAP_G_HEAD, cur, st));
    for (int l = 0; l <= 3; ++l) {            // decoder levels 0 (conv9) .. 3 (conv6)
        const int iu = L_UP3 + 3 * (3 - l);
        const int H = P.Hl[l], W = P.Wl[l], C = chan(l);
        // conv_2 of the level: input da[l]
        bd.wgrad(gs(cur), S_DA + l, -1);
        RC(conv_wgrad<T>(cur, C, B(P.da[l]), C, nullptr, 0, C, grd + P.L[iu + 2].w_off, grd + P.L[iu + 2].b_off, part, N, H, W, st));
        RC(marks.done(P, iu + 2, st));
        RC(bd.clear(gs(oth))); bd.bwd_data(gs(cur), S_W + iu + 2, gs(oth), -1);
        RC(conv_bwd_data<T>(cur, B(P.wp_bwd[iu + 2]), oth, nullptr, C, B(P.da[l]), nullptr, N, H, W, C, C, st, cd.da[l]));
        RC(tap.copy(TAP_DEC + 4 * l, oth, st));
        swap();
        // conv_1: input cat[up[l], eb[l]] -> d_up (raw) in oth, skip grad (raw) in skip[l]
        bd.wgrad(gs(cur), S_UP + l, S_EB + l);
        RC(conv_wgrad<T>(cur, C, B(P.up[l]), C, B(P.eb[l]), C, 2 * C, grd + P.L[iu + 1].w_off, grd + P.L[iu + 1].b_off, part, N, H, W, st));
        RC(marks.done(P, iu + 1, st));
        RC(bd.clear(gs(oth))); bd.bwd_data(gs(cur), S_W + iu + 1, gs(oth), S_SKIP + l);
        RC(conv_bwd_data<T>(cur, B(P.wp_bwd[iu + 1]), oth, B(P.skip[l]), C, nullptr, nullptr, N, H, W, 2 * C, C, st));
        RC(tap.copy(TAP_DEC + 4 * l + 1, oth, st));
        RC(tap.copy(TAP_DEC + 4 * l + 2, B(P.skip[l]), st));
        swap();
        // transposed conv: input src (level l+1, 2C channels), output grad = cur (d_up)
        const T* src = l == 3 ? B(P.eb[4]) : B(P.db[l + 1]);
        bd.wgrad(l == 3 ? S_EB + 4 : S_DB + l + 1, gs(cur), -1);
        RC(convt_wgrad<T>(src, cur, grd + P.L[iu].w_off, grd + P.L[iu].b_off, part, N, P.Hl[l + 1], P.Wl[l + 1], 2 * C, C, st));
        RC(marks.done(P, iu, st));
        RC(bd.clear(gs(oth))); bd.bwd_data(gs(cur), S_W + iu, gs(oth), -1);
        RC(convt_bwd_data<T>(cur, B(P.wp_bwd[iu]), src, oth, N, P.Hl[l + 1], P.Wl[l + 1], 2 * C, C, st));
        RC(tap.copy(TAP_DEC + 4 * l + 3, oth, st));
        swap();
    }
    // cur = pre-activation grad of conv5_2 (level 4)
    for (int l = 4; l >= 0; --l) {
        const int H = P.Hl[l], W = P.Wl[l], C = chan(l);
        const int ia = 2 * l, ib = 2 * l + 1;
        bd.wgrad(gs(cur), S_EA + l, -1);
        RC(conv_wgrad<T>(cur, C, B(P.ea[l]), C, nullptr, 0, C, grd + P.L[ib].w_off, grd + P.L[ib].b_off, part, N, H, W, st));
        RC(marks.done(P, ib, st));
        RC(bd.clear(gs(oth))); bd.bwd_data(gs(cur), S_W + ib, gs(oth), -1);
        RC(conv_bwd_data<T>(cur, B(P.wp_bwd[ib]), oth, nullptr, C, B(P.ea[l]), nullptr, N, H, W, C, C, st, cd.ea[l]));
        RC(tap.copy(TAP_ENC + 3 * (4 - l), oth, st));
        swap();
        if (l == 0) {
            if (cur != B(P.*GRAD_CONV1_1)) return ELD_EINVAL;      // one swap more or less above: GRAD_CONV1_1 moves with it
            if (P.in_ch <= 4)
                RC(launch_conv_first_wgrad(cur, fused.x ? fused.x : ws + P.x16, grd + P.L[ia].w_off, grd + P.L[ia].b_off, part, N, P.in_ch, H, W, st, g_algo == 1));
            else {      // the zero-padded NHWC input the forward left in ws + P.x16; only the in_ch real channels are written to dw
                bd.wgrad(gs(cur), S_X, -1);
                RC(conv_wgrad<T>(cur, C, B(P.x16), E::x_pad, nullptr, 0, P.in_ch, grd + P.L[ia].w_off, grd + P.L[ia].b_off, part, N, H, W, st));
            }
            RC(marks.done(P, ia, st));
            break;
        }
        const int Cp = chan(l - 1);
        bd.wgrad(gs(cur), S_EB + l - 1, -1);                 // pooled activations are bounded by their source's bound
        RC(conv_wgrad<T>(cur, C, B(P.pool[l - 1]), Cp, nullptr, 0, Cp, grd + P.L[ia].w_off, grd + P.L[ia].b_off, part, N, H, W, st));
        RC(marks.done(P, ia, st));
        RC(bd.clear(gs(oth))); bd.bwd_data(gs(cur), S_W + ia, gs(oth), -1);
        RC(conv_bwd_data<T>(cur, B(P.wp_bwd[ia]), oth, nullptr, Cp, nullptr, nullptr, N, H, W, Cp, C, st));      // d_pool (raw)
        RC(tap.copy(TAP_ENC + 3 * (4 - l) + 1, oth, st));
        swap();
        if (cd.eb[l - 1])
            RC(launch_maxpool_bwd_codes(cd.pc[l - 1], cd.eb[l - 1], cur, B(P.skip[l - 1]), oth, N, H, W, Cp, st));
        else
            RC(launch_maxpool_bwd(B(P.eb[l - 1]), cur, B(P.skip[l - 1]), oth, N, H, W, Cp, st));
        RC(bd.clear(gs(oth))); RC(bd.measure(oth, (size_t)N * 4 * H * W * Cp, gs(oth)));
        RC(tap.copy(TAP_ENC + 3 * (4 - l) + 2, oth, st));
        swap();
    }
    return 0;
}

}  // namespace

// ====================================================================================================
// C ABI
// ====================================================================================================
extern "C" int eld_unet_param_offsets(int in_ch, int out_ch, int64_t* offsets) {
    if (!offsets || in_ch < 1 || in_ch > 16 || out_ch < 1 || out_ch > 16) return ELD_EINVAL;
    LayerDef L[NLAYERS];
    const size_t n = build_layers(in_ch, out_ch, L);
    for (int i = 0; i < NLAYERS; ++i) { offsets[2 * i] = (int64_t)L[i].w_off; offsets[2 * i + 1] = (int64_t)L[i].b_off; }
    offsets[ELD_UNET_NTENSORS] = (int64_t)n;
    return 0;
}

extern "C" size_t eld_unet_workspace_bytes(int N, int H, int W, int in_ch, int out_ch) {
    Plan P;
    if (make_plan(P, N, H, W, in_ch, out_ch)) return 0;
    return P.total * sizeof(float);
}

// Which forward last filled a workspace (host call order = stream order for calls on one stream): eld_unet_backward_ex with dout == NULL consumes
// the gradient buffer and the head partials that ONLY eld_unet_forward_loss_ex leaves there, for exactly its N / H / W / precision.  Keyed by the
// workspace pointer; a plain forward on the same workspace clears the entry.  Host bookkeeping only: no device read, no synchronisation.
namespace {
struct HeadState { int N, H, W, in_ch, out_ch, precision; const float* x; };
// Which slope-code regions the last forward on a workspace filled, and for which problem (FusedFwd::codes): same bookkeeping, for EVERY forward
struct CodesState { int N, H, W, in_ch, out_ch, precision; unsigned have; };
// One table for both, keyed by the workspace pointer.  Workspaces come and go with their owners, so the table is bounded -- by evicting the ONE
// least recently touched entry, never by clearing it: an entry that is still between its forward and its backward is by construction among the most
// recently touched ones (it would take WS_STATE_MAX other workspaces run in between to push it out).  What a lost entry costs: no codes entry sends
// the backward to the saved activations (same bits); no head entry makes the dout == NULL backward fail with ELD_EINVAL.
struct WsState { HeadState head; bool has_head = false; CodesState codes; bool has_codes = false; unsigned long long stamp = 0; };
constexpr size_t WS_STATE_MAX = 256;
std::mutex g_head_mu;
std::unordered_map<const void*, WsState> g_ws_state;
unsigned long long g_ws_clock = 0;
WsState& ws_state_touch(const void* ws) {          // caller holds g_head_mu
    auto it = g_ws_state.find(ws);
    if (it == g_ws_state.end()) {
        if (g_ws_state.size() >= WS_STATE_MAX) {
            auto old = g_ws_state.begin();
            for (auto j = g_ws_state.begin(); j != g_ws_state.end(); ++j) if (j->second.stamp < old->second.stamp) old = j;
            g_ws_state.erase(old);
        }
        it = g_ws_state.emplace(ws, WsState()).first;
    }
    it->second.stamp = ++g_ws_clock;
    return it->second;
}
void ws_state_drop_if_empty(const void* ws) {       // caller holds g_head_mu
    const auto it = g_ws_state.find(ws);
    if (it != g_ws_state.end() && !it->second.has_head && !it->second.has_codes) g_ws_state.erase(it);
}
void codes_state_set(const void* ws, const CodesState& cs) {
    std::lock_guard<std::mutex> lk(g_head_mu);
    if (cs.have == 0) {
        const auto it = g_ws_state.find(ws);
        if (it != g_ws_state.end()) { it->second.has_codes = false; ws_state_drop_if_empty(ws); }
        return;
    }
    WsState& w = ws_state_touch(ws);
    w.codes = cs; w.has_codes = true;
}
unsigned codes_state_get(const void* ws, int N, int H, int W, int in_ch, int out_ch, int precision) {
    std::lock_guard<std::mutex> lk(g_head_mu);
    const auto it = g_ws_state.find(ws);
    if (it == g_ws_state.end() || !it->second.has_codes) return 0;
    it->second.stamp = ++g_ws_clock;
    const CodesState& c = it->second.codes;
    return c.N == N && c.H == H && c.W == W && c.in_ch == in_ch && c.out_ch == out_ch && c.precision == precision ? c.have : 0u;
}
void head_state_set(const void* ws, const HeadState* st) {
    std::lock_guard<std::mutex> lk(g_head_mu);
    if (st) {
        WsState& w = ws_state_touch(ws);
        w.head = *st; w.has_head = true;
    } else {
        const auto it = g_ws_state.find(ws);
        if (it != g_ws_state.end()) { it->second.has_head = false; ws_state_drop_if_empty(ws); }
    }
}
char* g_tap_buf = nullptr;          // eld_debug_unet_grad_tap (under g_head_mu)
size_t g_tap_bytes = 0;
bool head_state_is(const void* ws, HeadState& want) {      // fills want.x (the fused forward's input tensor) on a match
    std::lock_guard<std::mutex> lk(g_head_mu);
    const auto it = g_ws_state.find(ws);
    if (it == g_ws_state.end() || !it->second.has_head) return false;
    it->second.stamp = ++g_ws_clock;
    const HeadState& h = it->second.head;
    if (!(h.N == want.N && h.H == want.H && h.W == want.W && h.in_ch == want.in_ch && h.out_ch == want.out_ch && h.precision == want.precision)) return false;
    want.x = h.x;
    return true;
}
}  // namespace

static int unet_entry_checks(Plan& P, const void* a, const void* b, const void* c, const void* ws, size_t ws_bytes, int N, int H, int W, int in_ch, int out_ch) {
    RC(make_plan(P, N, H, W, in_ch, out_ch));
    if (!a || !b || !c || !ws) return ELD_EINVAL;
    if (ws_bytes < P.total * sizeof(float)) return ELD_EWS;
    return 0;
}

static int unet_forward_entry(const float* x, const float* params, float* out, void* ws, size_t ws_bytes, int N, int H, int W,
                              int in_ch, int out_ch, int precision, int fp32_algo, void* stream, bool infer) {
    if (N == 0) return 0;
    if ((precision != 0 && precision != 1) || fp32_algo > 2) return ELD_EINVAL;
    Plan P;
    RC(unet_entry_checks(P, x, params, out, ws, ws_bytes, N, H, W, in_ch, out_ch));
    AlgoScope scope(fp32_algo);
    head_state_set(ws, nullptr);      // whatever fused head state the workspace held is overwritten
    unsigned have = 0;
    const int rc = precision == 1 ? unet_forward<bf16_t>(P, x, params, out, (float*)ws, as_stream(stream), nullptr, &have, infer)
                                  : unet_forward<float>(P, x, params, out, (float*)ws, as_stream(stream), nullptr, &have, infer);
    codes_state_set(ws, CodesState{N, H, W, in_ch, out_ch, precision, rc == 0 ? (infer ? (unsigned)CODES_INFER : have) : 0u});
    return rc;
}
extern "C" int eld_unet_forward_ex(const float* x, const float* params, float* out, void* ws, size_t ws_bytes, int N, int H, int W,
                                   int in_ch, int out_ch, int precision, int fp32_algo, void* stream) {
    return unet_forward_entry(x, params, out, ws, ws_bytes, N, H, W, in_ch, out_ch, precision, fp32_algo, stream, false);
}
extern "C" int eld_unet_infer_ex(const float* x, const float* params, float* out, void* ws, size_t ws_bytes, int N, int H, int W,
                                 int in_ch, int out_ch, int precision, int fp32_algo, void* stream) {
    return unet_forward_entry(x, params, out, ws, ws_bytes, N, H, W, in_ch, out_ch, precision, fp32_algo, stream, true);
}

extern "C" int eld_unet_forward_loss_ex(const float* x, const float* params, const float* target, float* out, float* loss, void* ws, size_t ws_bytes,
                                        int N, int H, int W, int in_ch, int out_ch, int precision, int fp32_algo, int loss_kind, float grad_scale, void* stream) {
    if (N == 0) return 0;
    if ((precision != 0 && precision != 1) || fp32_algo > 2 || (loss_kind != 0 && loss_kind != 1) || !target || !loss) return ELD_EINVAL;
    Plan P;
    RC(unet_entry_checks(P, x, params, out, ws, ws_bytes, N, H, W, in_ch, out_ch));
    AlgoScope scope(fp32_algo);
    const HeadLoss hl = {target, loss, loss_kind, grad_scale};
    head_state_set(ws, nullptr);
    unsigned have = 0;
    const int rc = precision == 1 ? unet_forward<bf16_t>(P, x, params, out, (float*)ws, as_stream(stream), &hl, &have)
                                  : unet_forward<float>(P, x, params, out, (float*)ws, as_stream(stream), &hl, &have);
    codes_state_set(ws, CodesState{N, H, W, in_ch, out_ch, precision, rc == 0 ? have : 0u});
    if (rc == 0) { const HeadState hs = {N, H, W, in_ch, out_ch, precision, x}; head_state_set(ws, &hs); }
    return rc;
}
extern "C" int eld_unet_backward_ex(const float* dout, const float* params, float* grads, void* ws, size_t ws_bytes, int N, int H, int W,
                                    int in_ch, int out_ch, int precision, int fp32_algo, const int64_t* bucket_start, void* const* bucket_event,
                                    int n_buckets, void* stream) {
    if (N == 0) return 0;
    if ((precision != 0 && precision != 1) || fp32_algo > 2) return ELD_EINVAL;
    Plan P;
    RC(unet_entry_checks(P, dout ? (const void*)dout : (const void*)params, params, grads, ws, ws_bytes, N, H, W, in_ch, out_ch));      // dout == NULL: the head's share was done by eld_unet_forward_loss_ex
    if (n_buckets < 0 || (n_buckets > 0 && (!bucket_start || !bucket_event))) return ELD_EINVAL;
    // dout == NULL is only meaningful right after eld_unet_forward_loss_ex on this workspace with the same problem: anything else would hand back
    // stale head gradients without a sign of trouble
    FusedFwd fused;
    {
        HeadState hs = {N, H, W, in_ch, out_ch, precision, nullptr};
        const bool after_fused = head_state_is(ws, hs);
        if (!dout && !after_fused) return ELD_EINVAL;
        // An explicit dout after the fused-loss forward is a valid call order too (the head is then recomputed from dout): that forward left the
        // input with the caller instead of copying it into the workspace, so the first layer's weight gradient must read it there as well.
        if (after_fused) fused.x = in_ch <= 4 ? hs.x : nullptr;      // (more input planes: the forward converted x to NHWC16 in the workspace)
        fused.packed = !dout;                                         // with an explicit dout the backward packs its own weights (params may have changed)
        fused.codes = codes_state_get(ws, N, H, W, in_ch, out_ch, precision);
        if (fused.codes & CODES_INFER) return ELD_EINVAL;               // the last forward on this workspace was eld_unet_infer_ex: it kept nothing for a backward
    }
    for (int k = 0; k < n_buckets; ++k)
        if (!bucket_event[k] || bucket_start[k] < 0 || (k > 0 && bucket_start[k] <= bucket_start[k - 1]) || (size_t)bucket_start[k] >= P.nparams) return ELD_EINVAL;
    BucketMarks marks;
    marks.start = bucket_start; marks.event = bucket_event; marks.n = n_buckets;
    GradTap tap;
    {   // the debug tap (eld_debug_unet_grad_tap; unset outside the tests): its refusals come before any launch
        std::lock_guard<std::mutex> lk(g_head_mu);
        if (g_tap_buf) {
            tap.plan(P, precision);
            if (g_tap_bytes < tap.total) return ELD_EINVAL;
            hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
            if (hipStreamIsCapturing(as_stream(stream), &cs) != hipSuccess) { (void)hipGetLastError(); return ELD_ENOTSUP; }      // (the legacy stream beside a capture: not tappable either)
            if (cs != hipStreamCaptureStatusNone) return ELD_ENOTSUP;        // a graph must not bake the debug copies in
            tap.buf = g_tap_buf;
        }
    }
    AlgoScope scope(fp32_algo);
    const int rc = precision == 1 ? unet_backward<bf16_t>(P, dout, params, grads, (float*)ws, as_stream(stream), marks, fused, tap)
                                  : unet_backward<float>(P, dout, params, grads, (float*)ws, as_stream(stream), marks, fused, tap);
    if (rc) return rc;
    return marks.next == n_buckets ? 0 : ELD_EINVAL;
}

// the round-1 entry points: the fp32 product scheme is the process default (eld_conv_fp32_algo) at the time of EACH call
extern "C" int eld_unet_forward(const float* x, const float* params, float* out, void* ws, size_t ws_bytes, int N, int H, int W,
                                int in_ch, int out_ch, void* stream) {
    return eld_unet_forward_ex(x, params, out, ws, ws_bytes, N, H, W, in_ch, out_ch, 0, -1, stream);
}
extern "C" int eld_unet_forward_bf16(const float* x, const float* params, float* out, void* ws, size_t ws_bytes, int N, int H, int W,
                                     int in_ch, int out_ch, void* stream) {
    return eld_unet_forward_ex(x, params, out, ws, ws_bytes, N, H, W, in_ch, out_ch, 1, -1, stream);
}
extern "C" int eld_unet_backward(const float* dout, const float* params, float* grads, void* ws, size_t ws_bytes, int N, int H, int W,
                                 int in_ch, int out_ch, void* stream) {
    return eld_unet_backward_ex(dout, params, grads, ws, ws_bytes, N, H, W, in_ch, out_ch, 0, -1, nullptr, nullptr, 0, stream);
}
extern "C" int eld_unet_backward_bf16(const float* dout, const float* params, float* grads, void* ws, size_t ws_bytes, int N, int H, int W,
                                      int in_ch, int out_ch, void* stream) {
    return eld_unet_backward_ex(dout, params, grads, ws, ws_bytes, N, H, W, in_ch, out_ch, 1, -1, nullptr, nullptr, 0, stream);
}
extern "C" int eld_unet_backward_buckets(const float* dout, const float* params, float* grads, void* ws, size_t ws_bytes, int N, int H, int W,
                                         int in_ch, int out_ch, int precision, const int64_t* bucket_start, void* const* bucket_event,
                                         int n_buckets, void* stream) {
    return eld_unet_backward_ex(dout, params, grads, ws, ws_bytes, N, H, W, in_ch, out_ch, precision, -1, bucket_start, bucket_event, n_buckets, stream);
}

extern "C" void eld_debug_unet_grad_tap(void* buf, size_t bytes) {
    std::lock_guard<std::mutex> lk(g_head_mu);
    g_tap_buf = (char*)buf; g_tap_bytes = buf ? bytes : 0;
}
extern "C" int eld_debug_unet_grad_tap_layout(int N, int H, int W, int in_ch, int out_ch, int precision, int stage, size_t* offset, int* channels, int* level,
                                              int* dtype) {
    if (!offset || !channels || !level || !dtype || (precision != 0 && precision != 1)) return ELD_EINVAL;
    Plan P;
    RC(make_plan(P, N, H, W, in_ch, out_ch));
    int ch, lev;
    if (!tap_stage_shape(stage, ch, lev)) return ELD_EINVAL;
    GradTap t;
    t.plan(P, precision);
    *offset = t.off[stage]; *channels = ch; *level = lev; *dtype = precision;
    return 0;
}
extern "C" size_t eld_debug_unet_grad_tap_bytes(int N, int H, int W, int in_ch, int out_ch, int precision) {
    Plan P;
    if ((precision != 0 && precision != 1) || make_plan(P, N, H, W, in_ch, out_ch)) return 0;
    GradTap t;
    t.plan(P, precision);
    return t.total;
}
extern "C" int eld_debug_unet_codes(const void* ws) {
    std::lock_guard<std::mutex> lk(g_head_mu);
    const auto it = g_ws_state.find(ws);
    return it == g_ws_state.end() || !it->second.has_codes ? -1 : (int)it->second.codes.have;
}

extern "C" int eld_debug_ws_state_entries(void) { std::lock_guard<std::mutex> lk(g_head_mu); return (int)g_ws_state.size(); }

extern "C" void eld_debug_conv_prof(void* buf) { conv_x3_set_prof((unsigned long long*)buf); }

extern "C" int eld_conv_fp32_algo(int algo) { return conv_fp32_algo(algo); }

extern "C" size_t eld_l1_workspace_bytes(void) { return l1_ws_floats() * sizeof(float); }

extern "C" int eld_l1_loss(const float* out, const float* target, float* dout, float* loss, void* ws, size_t n, float grad_scale, void* stream) {
    if (!out || !target || !loss || !ws || n == 0) return ELD_EINVAL;
    return launch_l1(out, target, dout, loss, (float*)ws, n, grad_scale, as_stream(stream));
}

extern "C" int eld_mse_loss(const float* out, const float* target, float* dout, float* loss, void* ws, size_t n, float grad_scale, void* stream) {
    if (!out || !target || !loss || !ws || n == 0) return ELD_EINVAL;
    return launch_mse(out, target, dout, loss, (float*)ws, n, grad_scale, as_stream(stream));
}

extern "C" int eld_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n, double lr, double beta1,
                             double beta2, double eps, double weight_decay, int step, double grad_scale, void* stream) {
    if (n == 0) return 0;
    if (!params || !grads || !exp_avg || !exp_avg_sq || step < 1) return ELD_EINVAL;
    return launch_adam(params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale, as_stream(stream));
}

// ---- single layers -----------------------------------------------------------------------------------
extern "C" size_t eld_layer_workspace_bytes(int N, int H, int W, int Cin, int Cout) {
    if (N < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1) return 0;
    const int cinp = (Cin + 15) / 16 * 16;
    size_t f = (size_t)9 * Cout * cinp * 2 + 64;                            // one packed weight set (fp32 or pre-split slabs)
    size_t p = 0, q;
    if (Cout % 32 == 0) { q = wgrad_floats_max(CONV_3X3, Cout, Cin, N, H, W); p = q > p ? q : p; }
    if (Cin % 32 == 0) { q = wgrad_floats_max(CONV_GATHER2X2, Cin, Cout, N, H, W); p = q > p ? q : p; }
    q = colsum_ws_floats(Cout > Cin ? Cout : Cin); p = q > p ? q : p;
    return (align_up(f, 64) + align_up(p, 64) + 64) * sizeof(float);      // + 64 operand-bound slots (conv_fp32_algo 2)
}

// operand bounds of a single-layer call under conv_fp32_algo 2: slots 0..2 = inputs (a, b, c), 3..4 = outputs
static int layer_amax(void* ws, size_t ws_bytes, hipStream_t st, const float* a, size_t na, const float* b, size_t nb, const float* c, size_t nc, float** slots) {
    *slots = nullptr;
    if (g_algo != 2) return 0;
    float* am = (float*)ws + ws_bytes / sizeof(float) - 64;
    if (hipMemsetAsync(am, 0, 64 * sizeof(float), st) != hipSuccess) return (int)hipGetLastError();
    if (a) RC(launch_absmax(a, na, am + 0, st));
    if (b) RC(launch_absmax(b, nb, am + 1, st));
    if (c) RC(launch_absmax(c, nc, am + 2, st));
    *slots = am;
    return 0;
}

static int layer_ws(void* ws, size_t ws_bytes, int N, int H, int W, int Cin, int Cout, float** pack, float** part) {
    const size_t need = eld_layer_workspace_bytes(N, H, W, Cin, Cout);
    if (!ws || need == 0) return ELD_EINVAL;
    if (ws_bytes < need) return ELD_EWS;
    const int cinp = (Cin + 15) / 16 * 16;
    *pack = (float*)ws;
    *part = (float*)ws + align_up((size_t)9 * Cout * cinp * 2 + 64, 64);
    return 0;
}

// one layer's reference-layout fp32 weights -> the packed layout its kernel family reads, as pack_weights does for the same launch: a one-job pack_all launch.
// bf16: round to nearest even (bfdbn / bfgbn: the DMA kernels' slab width from bfd_slab_bn / bfg_slab_bn); fp32: plain, or the pre-split slabs of width x3bn.
// The channel rules of the callers give the groups of eight k-channels pack_all_kernel works in.
static int pack_one(const float* w, float* pack, int kind, int Cout, int Cin, int T, int bf16, int x3bn, int bfdbn, int bfgbn, hipStream_t st) {
    PackJobs jobs;
    jobs.n = 1;
    PackJob J = {};
    J.kind = kind; J.Cout = Cout; J.Cin = Cin; J.Cinp = Cin; J.T = T; J.bf16 = bf16; J.x3bn = x3bn; J.bfdbn = bfdbn; J.bfgbn = bfgbn;
    jobs.job[0] = J;
    return launch_pack_all(jobs, w, pack, st);
}

extern "C" int eld_conv3x3_forward(const float* in0, int C0, const float* in1, int C1, const float* w, const float* bias, float* out, int N,
                                   int H, int W, int Cout, int lrelu, void* ws, size_t ws_bytes, void* stream) {
    if (N == 0) return 0;
    AlgoScope scope(-1);
    if (!in0 || !w || !bias || !out || (C0 + C1) % 16 || C0 % 16 || Cout % 32) return ELD_EINVAL;
    float *pack, *part;
    RC(layer_ws(ws, ws_bytes, N, H, W, C0 + C1, Cout, &pack, &part));
    hipStream_t st = as_stream(stream);
    RC(pack_one(w, pack, PACK_CONV_FWD, Cout, C0 + C1, 9, 0, g_algo == 1 ? x3_slab_bn(Cout, N, H, W) : 0, 0, 0, st));
    float* am;
    RC(layer_amax(ws, eld_layer_workspace_bytes(N, H, W, C0 + C1, Cout), st, in0, (size_t)N * H * W * C0, in1, (size_t)N * H * W * C1, pack, (size_t)9 * Cout * (C0 + C1), &am));
    if (am) { g_am.in0 = am; g_am.in1 = in1 ? am + 1 : nullptr; g_am.w = am + 2; g_am.out0 = am + 3; }
    return conv_fwd(in0, C0, in1, C1, pack, bias, out, N, H, W, Cout, lrelu, st);
}

extern "C" int eld_conv3x3_backward_data(const float* g, const float* w, float* din0, float* din1, int split, const float* act0, const float* act1,
                                         int N, int H, int W, int Cin, int Cout, void* ws, size_t ws_bytes, void* stream) {
    if (N == 0) return 0;
    AlgoScope scope(-1);
    if (!g || !w || !din0 || Cin % 32 || Cout % 16 || split % 32 || split > Cin || (split < Cin && !din1)) return ELD_EINVAL;
    float *pack, *part;
    RC(layer_ws(ws, ws_bytes, N, H, W, Cin, Cout, &pack, &part));
    hipStream_t st = as_stream(stream);
    RC(pack_one(w, pack, PACK_CONV_BWD, Cout, Cin, 9, 0, g_algo == 1 ? x3_slab_bn(Cin, N, H, W) : 0, 0, 0, st));
    float* am;
    RC(layer_amax(ws, eld_layer_workspace_bytes(N, H, W, Cin, Cout), st, g, (size_t)N * H * W * Cout, nullptr, 0, pack, (size_t)9 * Cout * Cin, &am));
    if (am) { g_am.in0 = am; g_am.w = am + 2; g_am.out0 = am + 3; g_am.out1 = am + 4; }
    return conv_bwd_data(g, pack, din0, din1, split, act0, act1, N, H, W, Cin, Cout, st);
}

extern "C" int eld_conv3x3_backward_weight(const float* g, const float* x0, int C0, const float* x1, int C1, float* dw, float* db, int N, int H,
                                           int W, int Cout, void* ws, size_t ws_bytes, void* stream) {
    if (N == 0) return 0;
    AlgoScope scope(-1);
    if (!g || !x0 || !dw || Cout % 32 || C0 % 4 || C1 % 4) return ELD_EINVAL;
    float *pack, *part;
    RC(layer_ws(ws, ws_bytes, N, H, W, C0 + C1, Cout, &pack, &part));
    float* am;
    RC(layer_amax(ws, eld_layer_workspace_bytes(N, H, W, C0 + C1, Cout), as_stream(stream), g, (size_t)N * H * W * Cout, x1, (size_t)N * H * W * C1, x0, (size_t)N * H * W * C0, &am));
    if (am) { g_am.in0 = am; g_am.in1 = x1 ? am + 1 : nullptr; g_am.w = am + 2; }
    return conv_wgrad(g, Cout, x0, C0, x1, C1, C0 + C1, dw, db, part, N, H, W, as_stream(stream));
}

extern "C" int eld_convt2x2_forward(const float* in, const float* w, const float* bias, float* out, int N, int H, int W, int Cin, int Cout,
                                    void* ws, size_t ws_bytes, void* stream) {
    if (N == 0) return 0;
    AlgoScope scope(-1);
    if (!in || !w || !bias || !out || Cin % 16 || Cout % 8) return ELD_EINVAL;
    float *pack, *part;
    RC(layer_ws(ws, ws_bytes, N, H, W, Cin, Cout, &pack, &part));
    hipStream_t st = as_stream(stream);
    RC(pack_one(w, pack, PACK_CONVT_FWD, Cout, Cin, 4, 0, 0, 0, 0, st));
    float* am;
    RC(layer_amax(ws, eld_layer_workspace_bytes(N, H, W, Cin, Cout), st, in, (size_t)N * H * W * Cin, nullptr, 0, pack, (size_t)4 * Cout * Cin, &am));
    if (am) { g_am.in0 = am; g_am.w = am + 2; g_am.out0 = am + 3; }
    return convt_fwd(in, pack, bias, out, N, H, W, Cin, Cout, st);
}

extern "C" int eld_convt2x2_backward_data(const float* dout, const float* w, const float* act, float* din, int N, int H, int W, int Cin, int Cout,
                                          void* ws, size_t ws_bytes, void* stream) {
    if (N == 0) return 0;
    AlgoScope scope(-1);
    if (!dout || !w || !din || Cin % 32 || Cout % 16) return ELD_EINVAL;
    float *pack, *part;
    RC(layer_ws(ws, ws_bytes, N, H, W, Cin, Cout, &pack, &part));
    hipStream_t st = as_stream(stream);
    RC(pack_one(w, pack, PACK_CONVT_BWD, Cout, Cin, 4, 0, 0, 0, 0, st));
    float* am;
    RC(layer_amax(ws, eld_layer_workspace_bytes(N, H, W, Cin, Cout), st, dout, (size_t)N * 4 * H * W * Cout, nullptr, 0, pack, (size_t)4 * Cout * Cin, &am));
    if (am) { g_am.in0 = am; g_am.w = am + 2; g_am.out0 = am + 3; }
    return convt_bwd_data(dout, pack, act, din, N, H, W, Cin, Cout, st);
}

extern "C" int eld_convt2x2_backward_weight(const float* in, const float* dout, float* dw, float* db, int N, int H, int W, int Cin, int Cout,
                                            void* ws, size_t ws_bytes, void* stream) {
    if (N == 0) return 0;
    AlgoScope scope(-1);
    if (!in || !dout || !dw || Cin % 32 || Cout % 4) return ELD_EINVAL;
    float *pack, *part;
    RC(layer_ws(ws, ws_bytes, N, H, W, Cin, Cout, &pack, &part));
    float* am;
    RC(layer_amax(ws, eld_layer_workspace_bytes(N, H, W, Cin, Cout), as_stream(stream), in, (size_t)N * H * W * Cin, nullptr, 0, dout, (size_t)N * 4 * H * W * Cout, &am));
    if (am) { g_am.in0 = am; g_am.w = am + 2; }
    return convt_wgrad(in, dout, dw, db, part, N, H, W, Cin, Cout, as_stream(stream));
}

extern "C" int eld_maxpool2x2_forward(const float* in, float* out, int N, int Ho, int Wo, int C, void* stream) {
    if (N == 0) return 0;
    if (!in || !out || C % 4) return ELD_EINVAL;
    return launch_maxpool_fwd(in, out, N, Ho, Wo, C, as_stream(stream));
}

extern "C" int eld_maxpool2x2_backward(const float* act, const float* dp, const float* skip, float* g, int N, int Ho, int Wo, int C, void* stream) {
    if (N == 0) return 0;
    if (!act || !dp || !g || C % 4) return ELD_EINVAL;
    return launch_maxpool_bwd(act, dp, skip, g, N, Ho, Wo, C, as_stream(stream));
}

// ---- single layers on NHWC bf16 tensors (test hooks of the bf16 network's dispatchers) -------------------------------------------------
// Each call packs the reference-layout fp32 weights as pack_weights does for the same launch (bf16, round to nearest even; the DMA kernels' slab
// width from bfd_slab_bn / bfg_slab_bn) and calls the dispatcher the bf16 U-Net calls, so the launch runs on the kernel family the network would use.
extern "C" int eld_conv3x3_forward_bf16(const uint16_t* in0, int C0, const uint16_t* in1, int C1, const float* w, const float* bias, uint16_t* out,
                                        uint16_t* pool_out, int N, int H, int W, int Cout, int lrelu, void* ws, size_t ws_bytes, void* stream) {
    if (N == 0) return 0;
    if (!in0 || !w || !bias || !out || C0 % 32 || C1 % 32 || (C1 && !in1) || Cout % 32) return ELD_EINVAL;
    float *pack, *part;
    RC(layer_ws(ws, ws_bytes, N, H, W, C0 + C1, Cout, &pack, &part));
    hipStream_t st = as_stream(stream);
    RC(pack_one(w, pack, PACK_CONV_FWD, Cout, C0 + C1, 9, 1, 0, bfd_slab_bn(Cout, C0 + C1, N, H, W), 0, st));
    return conv_fwd<bf16_t>(in0, C0, in1, C1, reinterpret_cast<const bf16_t*>(pack), bias, out, N, H, W, Cout, lrelu, st, pool_out);
}

extern "C" int eld_conv3x3_backward_data_bf16(const uint16_t* g, const float* w, uint16_t* din0, uint16_t* din1, int split, const uint16_t* act0,
                                              const uint16_t* act1, int N, int H, int W, int Cin, int Cout, void* ws, size_t ws_bytes, void* stream) {
    if (N == 0) return 0;
    if (!g || !w || !din0 || Cin % 32 || Cout % 32 || split < 32 || split % 32 || split > Cin || (split < Cin && !din1)) return ELD_EINVAL;
    float *pack, *part;
    RC(layer_ws(ws, ws_bytes, N, H, W, Cin, Cout, &pack, &part));
    hipStream_t st = as_stream(stream);
    RC(pack_one(w, pack, PACK_CONV_BWD, Cout, Cin, 9, 1, 0, bfd_slab_bn(Cin, Cout, N, H, W), 0, st));
    return conv_bwd_data<bf16_t>(g, reinterpret_cast<const bf16_t*>(pack), din0, din1, split, act0, act1, N, H, W, Cin, Cout, st);
}

extern "C" int eld_conv3x3_backward_weight_bf16(const uint16_t* g, const uint16_t* x0, int C0, const uint16_t* x1, int C1, float* dw, float* db, int N,
                                                int H, int W, int Cout, void* ws, size_t ws_bytes, void* stream) {
    if (N == 0) return 0;
    if (!g || !x0 || !dw || Cout % 32 || C0 % 8 || C1 % 8 || (C1 && (!x1 || C0 % 32))) return ELD_EINVAL;
    float *pack, *part;
    RC(layer_ws(ws, ws_bytes, N, H, W, C0 + C1, Cout, &pack, &part));
    return conv_wgrad<bf16_t>(g, Cout, x0, C0, x1, C1, C0 + C1, dw, db, part, N, H, W, as_stream(stream));
}

extern "C" int eld_convt2x2_forward_bf16(const uint16_t* in, const float* w, const float* bias, uint16_t* out, int N, int H, int W, int Cin, int Cout,
                                         void* ws, size_t ws_bytes, void* stream) {
    if (N == 0) return 0;
    if (!in || !w || !bias || !out || Cin % 32 || Cout % 8) return ELD_EINVAL;
    float *pack, *part;
    RC(layer_ws(ws, ws_bytes, N, H, W, Cin, Cout, &pack, &part));
    hipStream_t st = as_stream(stream);
    RC(pack_one(w, pack, PACK_CONVT_FWD, Cout, Cin, 4, 1, 0, 0, bfg_slab_bn(false, 4 * Cout, Cin, Cout, N, H, W), st));
    return convt_fwd<bf16_t>(in, reinterpret_cast<const bf16_t*>(pack), bias, out, N, H, W, Cin, Cout, st);
}

extern "C" int eld_convt2x2_backward_data_bf16(const uint16_t* dout, const float* w, const uint16_t* act, uint16_t* din, int N, int H, int W, int Cin,
                                               int Cout, void* ws, size_t ws_bytes, void* stream) {
    if (N == 0) return 0;
    if (!dout || !w || !din || Cin % 32 || Cout % 32) return ELD_EINVAL;
    float *pack, *part;
    RC(layer_ws(ws, ws_bytes, N, H, W, Cin, Cout, &pack, &part));
    hipStream_t st = as_stream(stream);
    RC(pack_one(w, pack, PACK_CONVT_BWD, Cout, Cin, 4, 1, 0, 0, bfg_slab_bn(true, Cin, Cout, 0, N, H, W), st));
    return convt_bwd_data<bf16_t>(dout, reinterpret_cast<const bf16_t*>(pack), act, din, N, H, W, Cin, Cout, st);
}

extern "C" int eld_convt2x2_backward_weight_bf16(const uint16_t* in, const uint16_t* dout, float* dw, float* db, int N, int H, int W, int Cin, int Cout,
                                                 void* ws, size_t ws_bytes, void* stream) {
    if (N == 0) return 0;
    if (!in || !dout || !dw || Cin % 32 || Cout % 8) return ELD_EINVAL;
    float *pack, *part;
    RC(layer_ws(ws, ws_bytes, N, H, W, Cin, Cout, &pack, &part));
    return convt_wgrad<bf16_t>(in, dout, dw, db, part, N, H, W, Cin, Cout, as_stream(stream));
}

extern "C" int eld_maxpool2x2_forward_bf16(const uint16_t* in, uint16_t* out, int N, int Ho, int Wo, int C, void* stream) {
    if (N == 0) return 0;
    if (!in || !out || C % 4) return ELD_EINVAL;
    return launch_maxpool_fwd(in, out, N, Ho, Wo, C, as_stream(stream));
}

extern "C" int eld_maxpool2x2_backward_bf16(const uint16_t* act, const uint16_t* dp, const uint16_t* skip, uint16_t* g, int N, int Ho, int Wo, int C,
                                            void* stream) {
    if (N == 0) return 0;
    if (!act || !dp || !g || C % 4) return ELD_EINVAL;
    return launch_maxpool_bwd(act, dp, skip, g, N, Ho, Wo, C, as_stream(stream));
}

extern "C" int eld_debug_unet_region(int N, int H, int W, int in_ch, int out_ch, int precision, int region, int level, size_t* offset, int* channels,
                                     int* dtype) {
    if (!offset || !channels || !dtype || (precision != 0 && precision != 1)) return ELD_EINVAL;
    Plan P;
    RC(make_plan(P, N, H, W, in_ch, out_ch));
    const bool full = region == ELD_REGION_EA || region == ELD_REGION_EB;
    if (level < 0 || level >= (full ? NLEV : NLEV - 1) || (region >= ELD_REGION_X16 && level != 0)) return ELD_EINVAL;
    size_t off;
    int ch = chan(level), dt = precision;
    switch (region) {
        case ELD_REGION_EA: off = P.ea[level]; break;
        case ELD_REGION_EB: off = P.eb[level]; break;
        case ELD_REGION_POOL: off = P.pool[level]; break;
        case ELD_REGION_UP: off = P.up[level]; break;
        case ELD_REGION_DA: off = P.da[level]; break;
        case ELD_REGION_DB: off = P.db[level]; break;
        case ELD_REGION_X16:
            off = P.x16;
            if (in_ch <= 4) { ch = in_ch; dt = 2; }          // the fp32 NCHW copy of the input (forwards other than eld_unet_forward_loss_ex)
            else ch = precision ? 32 : 16;
            break;
        case ELD_REGION_GRAD_CONV1_1:
            if (precision != 1) return ELD_ENOTSUP;
            off = P.*GRAD_CONV1_1; ch = 32;
            break;
        default: return ELD_EINVAL;
    }
    *offset = off * sizeof(float);
    *channels = ch;
    *dtype = dt;
    return 0;
}
