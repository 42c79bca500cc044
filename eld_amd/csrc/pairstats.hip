// pairstats.hip -- exact integer error-versus-signal sums of an estimate against a reference frame (eld_amd/evaluate.py).
//
//   eld_pair_level_stats_u16   est, ref uint16 mosaics [F,Hm,Wm] -> out[F][G][NB][4] = (n, sum s, sum e, sum e^2) per colour group and signal bin
// s = int(ref) - black[cell], e = int(est) - int(ref), bin = a pure integer function of ref (bin_of in levelbins.h; NB = 61).  Sites outside
// [0, Hc) x [0, Wc), sites flagged in the defect bitmap and cells of group -1 contribute nothing.  Integer adds only: any arrival order, any
// launch geometry gives the same bits.  e^2 <= 65535^2 < 2^32 and Hm Wm < 2^31, so sum e^2 < 2^63: every output fits int64.
//
// One pass, 4 bytes read per site.  A frame is read as a flat array in chunks of 8 sites: one 16-byte load of est and one of ref per lane.
//   * PS_ROWS   Wm % 8 == 0 and both stacks 16-byte aligned: a chunk lies inside one row, the row and the first column come from one
//               division per chunk, the 8 cells from a 12-entry row of a small LDS table, the 8 defect bits from one bitmap word.
//   * PS_FLAT   both stacks 16-byte aligned, any width: the same 16-byte loads over the aligned body of each frame; a chunk may straddle rows,
//               so every site derives its own (y, x).  The up to 7 + 7 sites before and after the aligned body of a frame (odd sizes move the
//               frame starts) are read one by one by a workgroup of their own.
//   * PS_SCALAR any alignment: one site per lane and turn, 2-byte loads.
// Accumulation.  A workgroup (512 threads) covers at most PS_SITES = 32768 sites of one frame, so its partial sums fit 32 bits (n, and
// |sum s|, |sum e| <= 32768 * 65535 < 2^31) except sum e^2 (64 bits): a table entry is 3 words + 1 double word, a table of G * NB <= 244
// entries 4880 bytes.  Contention (dark frames put nearly every site of a wave into one or two bins) is met twice:
//   * runs are merged in the lane: a lane keeps one pending (key, n, s, e, e^2) per column parity -- on a Bayer row the sites of one parity
//     share a colour -- and adds a site with the pending key in registers; only a change of key goes to the LDS.  The pending entries live
//     across the lane's chunks, so a constant region (clipped sky, black border, the all-in-one-bin frame) costs no LDS add at all.
//   * the workgroup holds PS_COPIES = 16 copies of the table and lane l adds to copy l % 16.  The copy stride is 2 modulo 32 words: one entry
//     of the 16 copies lies in 16 different even banks (the double words in all 32), so 64 lanes on one entry meet 4-way serialisation
//     instead of 64-way.  16 copies are 80000 bytes: two workgroups (16 waves) per CU.
// At its end a workgroup folds the copies and adds every non-zero sum to out[] with a 64-bit global integer atomic (at most 976 per 32768
// sites); out[] is zeroed by a kernel of this call first.  No floating point anywhere, no environment switch, no workspace.
#include "levelbins.h"
#include "mosaic_dev.h"

namespace {

constexpr int PT = 512;                          // threads per workgroup
constexpr int PS_TW = 4 * PS_NB;                 // table entries (G <= 4)
constexpr int PS_COPIES = 16;
constexpr int PS_QOFF = 3 * PS_TW;               // words n[TW], s[TW], e[TW], then TW double words of e^2 (732 is even: 8-byte aligned)
constexpr int PS_STRIDE = 1250;                  // >= 5 * TW = 1220, even, and 2 modulo 32
constexpr int PS_LDS_BYTES = PS_COPIES * PS_STRIDE * 4;
constexpr int PS_TURNS = 8;                      // chunks per lane
constexpr int PS_CHUNKS = PT * PS_TURNS;         // chunks per workgroup
constexpr int PS_SITES = PS_CHUNKS * 8;          // 32768: the bound behind the 32-bit partial sums
static_assert(PS_STRIDE >= 5 * PS_TW && PS_STRIDE % 32 == 2 && PS_QOFF % 2 == 0, "LDS layout");
static_assert((long long)PS_SITES * 65535 < (1ll << 31), "32-bit partial sums");

enum { PS_ROWS = 0, PS_FLAT = 1, PS_SCALAR = 2 };

struct PairStatArgs {
    const uint16_t* est;
    const uint16_t* ref;
    const uint32_t* bitmap;
    long long* out;
    int Hm, Wm, Hc, Wc, G, white, wpr;
    uint32_t hw, cpr;                            // sites per frame; PS_ROWS: chunks per row
    FastDiv dcpr, dwm;
    int32_t tab[36];                             // cell -> black | (group + 1) << 16
};

extern __shared__ unsigned long long ps_lds[];

// the pending run of one column parity
struct Run {
    int key;
    uint32_t n;
    int32_t s, e;
    unsigned long long q;
};

__device__ __forceinline__ void run_clear(Run& r) { r.key = -1; r.n = 0; r.s = 0; r.e = 0; r.q = 0; }

__device__ __forceinline__ void run_flush(uint32_t* __restrict__ tab, const Run& r) {
    if (r.key >= 0) {
        atomicAdd(tab + r.key, r.n);
        atomicAdd(tab + PS_TW + r.key, (uint32_t)r.s);
        atomicAdd(tab + 2 * PS_TW + r.key, (uint32_t)r.e);
        atomicAdd(reinterpret_cast<unsigned long long*>(tab + PS_QOFF) + r.key, r.q);
    }
}

// one site: t = the cell's table word, ok = inside the crop and not flagged
__device__ __forceinline__ void run_add(uint32_t* __restrict__ tab, Run& r, int est, int ref, int t, bool ok, int white) {
    const int g = (t >> 16) - 1;
    if (ok && g >= 0) {
        const int s = ref - (t & 0xFFFF), e = est - ref;
        const int key = g * PS_NB + bin_of(ref, s, white);
        const uint32_t q = (uint32_t)e * (uint32_t)e;            // e^2 <= 65535^2 < 2^32
        if (key == r.key) {
            r.n += 1; r.s += s; r.e += e; r.q += q;
        } else {
            run_flush(tab, r);
            r.key = key; r.n = 1; r.s = s; r.e = e; r.q = q;
        }
    }
}

template <int P, int MODE>
__global__ __launch_bounds__(PT) void pairstats_kernel(PairStatArgs a) {
    __shared__ int32_t s_tab[P * CELL_ROW];
    uint32_t* lds = reinterpret_cast<uint32_t*>(ps_lds);
    for (int i = threadIdx.x; i < PS_COPIES * PS_STRIDE; i += PT) lds[i] = 0;
    fill_cell_rows<P>(s_tab, a.tab);
    __syncthreads();
    uint32_t* tab = lds + (threadIdx.x & (PS_COPIES - 1)) * PS_STRIDE;
    const int f = blockIdx.y;
    const size_t fo = (size_t)f * a.hw;
    const uint16_t* fe = a.est + fo;
    const uint16_t* fr = a.ref + fo;
    const int white = a.white;
    Run run[2];
    run_clear(run[0]);
    run_clear(run[1]);

    // a site by its index in the frame: everything derived per site
    auto site = [&](uint32_t i, int est, int ref, Run& r) __attribute__((always_inline)) {
        const uint32_t y = fdiv_u32(i, a.dwm);
        const uint32_t x = i - y * (uint32_t)a.Wm;
        const uint32_t ym = cell_phase<P>(y), xm = cell_phase<P>(x);
        bool ok = (int)y < a.Hc && (int)x < a.Wc;
        if (a.bitmap) ok = ok && !defect_bit(a.bitmap, a.wpr, y, x);
        run_add(tab, r, est, ref, s_tab[ym * CELL_ROW + xm], ok, white);
    };

    if constexpr (MODE == PS_SCALAR) {
        const uint32_t i0 = blockIdx.x * (uint32_t)PS_SITES;
        const uint32_t i1 = min(i0 + (uint32_t)PS_SITES, a.hw);
        for (uint32_t i = i0 + threadIdx.x; i < i1; i += PT) site(i, fe[i], fr[i], run[0]);
    } else {
        // the aligned body of the frame: head sites before it, nch chunks, tail sites after it (PS_ROWS: head = tail = 0)
        const uint32_t head = MODE == PS_ROWS ? 0u : min((uint32_t)((8u - (uint32_t)(fo & 7u)) & 7u), a.hw);
        const uint32_t nch = (a.hw - head) >> 3;
        const uint32_t tail = a.hw - head - 8u * nch;
        const bool edge = MODE == PS_FLAT && blockIdx.x == gridDim.x - 1;   // PS_FLAT: the last workgroup of a frame reads its head and tail only
        const uint32_t c0 = blockIdx.x * (uint32_t)PS_CHUNKS;
        const uint32_t c1 = edge ? c0 : min(c0 + (uint32_t)PS_CHUNKS, nch);
#pragma unroll 2
        for (uint32_t ci = c0 + threadIdx.x; ci < c1; ci += PT) {
            const uint32_t i = head + 8u * ci;
            const uint4 qe = *reinterpret_cast<const uint4*>(fe + i);
            const uint4 qr = *reinterpret_cast<const uint4*>(fr + i);
            const uint32_t we[4] = {qe.x, qe.y, qe.z, qe.w}, wr[4] = {qr.x, qr.y, qr.z, qr.w};
            if constexpr (MODE == PS_ROWS) {
                const uint32_t y = fdiv_u32(ci, a.dcpr);
                const uint32_t x0 = (ci - y * a.cpr) * 8u;
                const int32_t* trow = cell_row<P>(s_tab, y, x0);
                uint32_t bad = 0;
                if (a.bitmap) bad = defect_bits(a.bitmap, a.wpr, y, x0);
                const bool rowin = (int)y < a.Hc;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int est = (int)code_of(we, j), ref = (int)code_of(wr, j);
                    const bool ok = rowin && (int)x0 + j < a.Wc && !((bad >> j) & 1u);
                    run_add(tab, run[j & 1], est, ref, trow[j], ok, white);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int est = (int)code_of(we, j), ref = (int)code_of(wr, j);
                    site(i + j, est, ref, run[j & 1]);
                }
            }
        }
        if (edge && threadIdx.x < head + tail) {
            const uint32_t i = threadIdx.x < head ? threadIdx.x : a.hw - tail + (threadIdx.x - head);
            site(i, fe[i], fr[i], run[0]);
        }
    }
    run_flush(tab, run[0]);
    run_flush(tab, run[1]);

    __syncthreads();
    long long* out = a.out + (size_t)f * a.G * (PS_NB * 4);
    const int tw = a.G * PS_NB;
    for (int k = threadIdx.x; k < tw; k += PT) {
        uint32_t n = 0;
        int32_t s = 0, e = 0;
        unsigned long long q = 0;
        for (int c = 0; c < PS_COPIES; ++c) {
            const uint32_t* t = lds + c * PS_STRIDE;
            n += t[k];
            s += (int32_t)t[PS_TW + k];
            e += (int32_t)t[2 * PS_TW + k];
            q += reinterpret_cast<const unsigned long long*>(t + PS_QOFF)[k];
        }
        unsigned long long* o = reinterpret_cast<unsigned long long*>(out + 4 * k);
        if (n) atomicAdd(o, (unsigned long long)n);
        if (s) atomicAdd(o + 1, (unsigned long long)(long long)s);
        if (e) atomicAdd(o + 2, (unsigned long long)(long long)e);
        if (q) atomicAdd(o + 3, q);
    }
}

template <int P, int MODE>
int launch_pairstats(const PairStatArgs& a, dim3 grid, hipStream_t s) {
    static EldAttrOnce once;
    const int rc = once.ensure(pairstats_kernel<P, MODE>, (size_t)PS_LDS_BYTES);
    if (rc) return rc;
    ELD_LAUNCH((pairstats_kernel<P, MODE>), grid, dim3(PT), (size_t)PS_LDS_BYTES, s, a);
    ELD_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" size_t eld_pair_level_stats_workspace_bytes(int F, int Hm, int Wm) {
    (void)F; (void)Hm; (void)Wm;
    return 0;                                                    // the sums meet in LDS and in out[] itself
}

extern "C" int eld_pair_level_stats_u16(const uint16_t* est, const uint16_t* ref, int F, int Hm, int Wm, int Hc, int Wc, int p, const int* group,
                                        int G, const int32_t* black, int white, const uint32_t* bitmap, int64_t* out, void* ws, size_t ws_bytes,
                                        void* stream) {
    if ((p != 2 && p != 6) || F < 0 || F > 65535 || Hm < 0 || Wm < 0 || Hc < 0 || Hc > Hm || Wc < 0 || Wc > Wm || G < 1 || G > 4) return ELD_EINVAL;
    if ((uint64_t)Hm * (uint64_t)Wm >= (1ull << 31) || !cell_groups_ok(p, group, G, black, white)) return ELD_EINVAL;
    (void)ws;
    if (ws_bytes < eld_pair_level_stats_workspace_bytes(F, Hm, Wm)) return ELD_EWS;
    if (F == 0) return 0;
    if (!out || ((uintptr_t)out & 7u)) return ELD_EINVAL;
    const bool empty = Hm == 0 || Wm == 0;
    if (!empty && (!est || !ref || ((uintptr_t)est & 1u) || ((uintptr_t)ref & 1u) || ((uintptr_t)bitmap & 3u))) return ELD_EINVAL;
    hipStream_t s = as_stream(stream);
    if (int rc = zero_u64(out, (size_t)F * G * PS_NB * 4, s)) return rc;
    if (empty || Hc == 0 || Wc == 0) return 0;
    PairStatArgs a;
    a.est = est; a.ref = ref; a.bitmap = bitmap; a.out = (long long*)out;
    a.Hm = Hm; a.Wm = Wm; a.Hc = Hc; a.Wc = Wc; a.G = G; a.white = white; a.wpr = bitmap_pitch(Wm);
    a.hw = (uint32_t)Hm * (uint32_t)Wm;
    pack_cell_tab(a.tab, p, group, black);
    const bool al16 = !(((uintptr_t)est | (uintptr_t)ref) & 15u);
    const int mode = !al16 ? PS_SCALAR : (Wm % 8 == 0 ? PS_ROWS : PS_FLAT);
    a.cpr = mode == PS_ROWS ? (uint32_t)(Wm / 8) : 1u;
    a.dcpr = make_fastdiv(a.cpr);
    a.dwm = make_fastdiv((uint32_t)Wm);
    // workgroups per frame: PS_SITES sites (PS_SCALAR) or PS_CHUNKS chunks each; PS_FLAT: one more for the frame's head and tail, so that no
    // workgroup exceeds PS_SITES sites
    const uint32_t units = mode == PS_SCALAR ? (a.hw + PS_SITES - 1) / PS_SITES : ((a.hw >> 3) + PS_CHUNKS - 1) / PS_CHUNKS + (mode == PS_FLAT ? 1u : 0u);
    const dim3 grid(units, (unsigned)F);
    if (p == 2) {
        if (mode == PS_ROWS) return launch_pairstats<2, PS_ROWS>(a, grid, s);
        if (mode == PS_FLAT) return launch_pairstats<2, PS_FLAT>(a, grid, s);
        return launch_pairstats<2, PS_SCALAR>(a, grid, s);
    }
    if (mode == PS_ROWS) return launch_pairstats<6, PS_ROWS>(a, grid, s);
    if (mode == PS_FLAT) return launch_pairstats<6, PS_FLAT>(a, grid, s);
    return launch_pairstats<6, PS_SCALAR>(a, grid, s);
}
