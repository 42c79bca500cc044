// noiselevel.hip -- exact integer tile sums for the noise level of a single raw frame (eld_amd/noiselevel.py).
//
//   eld_tile_noise_sums_u16   frames uint16 [F,Hm,Wm] -> out[F][nty][ntx][G][4] = (n, sum S9, sum r^2, sum dx^2 + dy^2) per tile and colour group
// A site (y, x), s <= y < Hc - s, s <= x < Wc - s, looks at the nine codes v[a][b] at (y + (a - 1) s, x + (b - 1) s): the same-colour
// neighbours at stride s.  It is eligible when the nine sites share one group >= 0, none is flagged in the defect bitmap and every code is
// > 0 and < white; then r = the 3 x 3 second difference (1 -2 1; -2 4 -2; 1 -2 1), dx = v12 - v10, dy = v21 - v01 and S9 = the nine
// codes minus their black levels.  Tile (ty, tx) owns the sites with (y - s) / 16s == ty, (x - s) / 16s == tx.  Integer adds only.
//
// One workgroup (256 threads) owns one tile and writes its 4 G sums: no atomics, no workspace, out[] needs no zeroing pass.
//   * stage   the tile and its halo of s, 18s x 18s codes, go to LDS as "code or 0": a code >= white, a flagged site, a cell of group -1 and
//             everything outside [0, Hc) x [0, Wc) become 0, which the rule "every code > 0" then refuses -- so the compute stage tests
//             nine values against 0 and nothing else, and the partial tiles at the bottom and the right need no case of their own (a site
//             with y >= Hc - s has the zero at y + s among its nine).  With the stack 16-byte aligned a row piece is read as the aligned
//             8-code chunks that cover it (any width: the chunks are aligned in the flat array, the codes outside the piece are dropped;
//             a chunk that would leave the stack is read code by code); otherwise 2-byte loads.
//   * sums    the nine cells of a site are a function of its cell (y % p, x % p): the host folds "the nine share a group" and the sum of
//             their nine black levels into one table word per cell.  Wave w takes the cells w, w + 4, ...; its lanes take the sites of
//             that cell in the tile (a lattice of pitch p), so the group is wave-uniform and a lane keeps one set of four accumulators.
//             When the group changes, and at the end, the wave folds its lanes (shuffles) into its own row of an LDS table.
//   * store   after a barrier thread j < 4 G adds the four waves' rows and stores out[..][j].
// Bounds: |r| <= 8 * 65535 < 2^20, r^2 < 2^38; dx^2 + dy^2 < 2^33; S9 < 2^20; a tile has at most (16 * 6)^2 = 9216 < 2^14 sites: every
// sum stays below 2^52.
#include "mosaic_dev.h"

namespace {

constexpr int NL_T = 256;                        // threads per workgroup
constexpr int NL_WAVES = NL_T / ELD_WAVE;
constexpr int NL_TS = 16;                        // tile side in units of the stride

struct NoiseTileArgs {
    const uint16_t* frames;
    const uint32_t* bitmap;
    long long* out;
    int Hm, Wm, Hc, Wc, G, white, wpr, ntx, nty;
    uint32_t hw;                                 // sites per frame
    unsigned long long total;                    // codes in the stack
    unsigned long long counted;                  // bit c: cell c has a group >= 0
    FastDiv dntx;
    int32_t tab[36];                             // cell -> sum of the nine black levels | (the nine's common group + 1) << 24, 0 in the top byte: not eligible
};

template <int P, int S, bool VEC>
__global__ __launch_bounds__(NL_T) void noise_tile_kernel(NoiseTileArgs a) {
    constexpr int SIDE = NL_TS * S;              // sites per tile side
    constexpr int RS = SIDE + 2 * S;             // staged codes per side
    constexpr int PITCH = RS + (RS & 1);         // even: a row starts on a 32-bit word
    constexpr int CPR = (RS + 7) / 8 + 1;        // aligned 8-code chunks that can cover RS codes at any phase
    __shared__ uint16_t s_v[RS * PITCH];
    __shared__ int32_t s_tab[P * P];
    __shared__ unsigned long long s_acc[NL_WAVES][4][4];

    const int tid = threadIdx.x;
    const uint32_t ty = fdiv_u32(blockIdx.x, a.dntx);
    const uint32_t tx = blockIdx.x - ty * (uint32_t)a.ntx;
    const int f = blockIdx.y;
    const int ys = (int)ty * SIDE, xs = (int)tx * SIDE;           // the staged region's first row and column (the tile's first site minus s)

    {
        uint32_t* z = reinterpret_cast<uint32_t*>(s_v);
        for (int i = tid; i < RS * PITCH / 2; i += NL_T) z[i] = 0;
        if (tid < P * P) s_tab[tid] = a.tab[tid];
        if (tid < NL_WAVES * 16) (&s_acc[0][0][0])[tid] = 0;
    }
    __syncthreads();

    // ---- stage: rows ys .. ys + RS - 1 below Hc, columns xs .. xs + RS - 1 below Wc
    const int rows = min(RS, a.Hc - ys), cols = min(RS, a.Wc - xs);
    const unsigned long long fo = (unsigned long long)f * a.hw;
    const int white = a.white;
    auto keep = [&](int code, uint32_t ym, int x, bool flagged) __attribute__((always_inline)) -> uint16_t {
        const uint32_t c = ym * P + cell_phase<P>((uint32_t)x);
        const bool ok = code < white && !flagged && ((a.counted >> c) & 1ull);
        return ok ? (uint16_t)code : (uint16_t)0;
    };
    if constexpr (VEC) {
        for (int t = tid; t < rows * CPR; t += NL_T) {
            const int ly = t / CPR, k = t - ly * CPR;
            const int y = ys + ly;
            const unsigned long long i0 = fo + (unsigned long long)y * a.Wm + xs;         // the piece is [i0, i0 + cols) of the flat stack
            const unsigned long long cb = (i0 & ~7ull) + 8ull * k;                        // this chunk's first code
            if (cb >= i0 + cols) continue;
            const int j0 = cb < i0 ? (int)(i0 - cb) : 0;                                  // the chunk's codes j0 .. j1 - 1 lie in the piece
            const int j1 = (int)min(8ull, i0 + cols - cb);
            const int xb = xs + (int)((long long)cb - (long long)i0);                     // the column of the chunk's code 0 (may lie before xs)
            unsigned long long bad = 0;
            if (a.bitmap) {                                                               // the up to 8 bits from column xb + j0 on lie in two words
                const int xf = xb + j0;
                const uint32_t* bw = a.bitmap + (size_t)y * a.wpr + (xf >> 5);
                bad = bw[0];
                if ((xf >> 5) + 1 < a.wpr) bad |= (unsigned long long)bw[1] << 32;
                bad >>= (xf & 31);
            }
            const uint32_t ym = cell_phase<P>((uint32_t)y);
            const int lx0 = (int)((long long)cb - (long long)i0);                         // the chunk's code j goes to column lx0 + j of the staged row
            uint16_t* row = s_v + ly * PITCH;
            if (cb + 8 > a.total) {                                                       // the stack's last, partial chunk: code by code
                for (int j = j0; j < j1; ++j) row[lx0 + j] = keep((int)a.frames[cb + j], ym, xb + j, (bad >> (j - j0)) & 1ull);
                continue;
            }
            const uint4 q = *reinterpret_cast<const uint4*>(a.frames + cb);
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (j >= j0 && j < j1) row[lx0 + j] = keep((int)code_of(w, j), ym, xb + j, (bad >> (j - j0)) & 1ull);
        }
    } else {
        for (int t = tid; t < rows * RS; t += NL_T) {
            const int ly = t / RS, lx = t - ly * RS;
            if (lx >= cols) continue;
            const int y = ys + ly, x = xs + lx;
            const bool flagged = a.bitmap && defect_bit(a.bitmap, a.wpr, y, x);
            s_v[ly * PITCH + lx] = keep((int)a.frames[fo + (unsigned long long)y * a.Wm + x], cell_phase<P>((uint32_t)y), x, flagged);
        }
    }
    __syncthreads();

    // ---- sums: wave w takes the cells w, w + 4, ...
    const int lane = tid & (ELD_WAVE - 1), wave = tid / ELD_WAVE;
    const int y0 = ys + S, x0 = xs + S;                                                   // the tile's first site
    const int py = (int)cell_phase<P>((uint32_t)y0), px = (int)cell_phase<P>((uint32_t)x0);
    int cur = -1;
    unsigned long long an = 0, as = 0, ar = 0, ad = 0;
    auto flush = [&]() __attribute__((always_inline)) {
        if (cur >= 0) {
#pragma unroll
            for (int m = ELD_WAVE / 2; m >= 1; m >>= 1) {         // four sums per step: wave_sum four times is another instruction stream
                an += __shfl_xor(an, m, ELD_WAVE);
                as += __shfl_xor(as, m, ELD_WAVE);
                ar += __shfl_xor(ar, m, ELD_WAVE);
                ad += __shfl_xor(ad, m, ELD_WAVE);
            }
            if (lane == 0) {
                s_acc[wave][cur][0] += an;
                s_acc[wave][cur][1] += as;
                s_acc[wave][cur][2] += ar;
                s_acc[wave][cur][3] += ad;
            }
        }
        an = as = ar = ad = 0;
    };
    for (int pos = wave; pos < P * P; pos += NL_WAVES) {
        const int t = s_tab[pos];
        const int g = (t >> 24) - 1;
        if (g < 0) continue;
        if (g != cur) {
            flush();
            cur = g;
        }
        const int b9 = t & 0xFFFFFF;
        const int cy = pos / P, cx = pos - cy * P;
        const int fy = (cy - py + P) % P, fx = (cx - px + P) % P;                         // the tile's first row and column of this cell
        const int ny = fy < SIDE ? (SIDE - fy + P - 1) / P : 0, nx = fx < SIDE ? (SIDE - fx + P - 1) / P : 0;
        for (int k = lane; k < ny * nx; k += ELD_WAVE) {
            const int ky = k / nx, kx = k - ky * nx;
            const uint16_t* v = s_v + (fy + ky * P) * PITCH + fx + kx * P;                // v[a * S * PITCH + b * S] = v[a][b]
            const int v00 = v[0], v01 = v[S], v02 = v[2 * S];
            const int v10 = v[S * PITCH], v11 = v[S * PITCH + S], v12 = v[S * PITCH + 2 * S];
            const int v20 = v[2 * S * PITCH], v21 = v[2 * S * PITCH + S], v22 = v[2 * S * PITCH + 2 * S];
            const bool ok = v00 && v01 && v02 && v10 && v11 && v12 && v20 && v21 && v22;
            if (ok) {
                const int r = v00 - 2 * v01 + v02 - 2 * v10 + 4 * v11 - 2 * v12 + v20 - 2 * v21 + v22;
                const int dx = v12 - v10, dy = v21 - v01;
                an += 1;
                as += (unsigned long long)(long long)(v00 + v01 + v02 + v10 + v11 + v12 + v20 + v21 + v22 - b9);
                ar += (unsigned long long)((long long)r * r);
                ad += (unsigned long long)((long long)dx * dx + (long long)dy * dy);
            }
        }
    }
    flush();
    __syncthreads();

    // ---- store
    if (tid < 4 * a.G) {
        unsigned long long v = 0;
#pragma unroll
        for (int w = 0; w < NL_WAVES; ++w) v += (&s_acc[w][0][0])[tid];
        a.out[(((size_t)f * a.nty + ty) * a.ntx + tx) * (size_t)(4 * a.G) + tid] = (long long)v;
    }
}

template <int P, int S>
int launch_noise_tiles(const NoiseTileArgs& a, bool vec, dim3 grid, hipStream_t s) {
    if (vec) ELD_LAUNCH((noise_tile_kernel<P, S, true>), grid, dim3(NL_T), 0, s, a);
    else ELD_LAUNCH((noise_tile_kernel<P, S, false>), grid, dim3(NL_T), 0, s, a);
    ELD_LAUNCH_CHECK();
    return 0;
}

int tiles_along(int n, int s) { return n > 2 * s ? (n - 2 * s + NL_TS * s - 1) / (NL_TS * s) : 0; }

}  // namespace

extern "C" size_t eld_tile_noise_workspace_bytes(int F, int Hm, int Wm) {
    (void)F; (void)Hm; (void)Wm;
    return 0;                                                    // a tile's sums meet in LDS; every entry of out[] has one writer
}

extern "C" int eld_tile_noise_sums_u16(const uint16_t* frames, int F, int Hm, int Wm, int Hc, int Wc, int p, int stride, const int* group, int G,
                                       const int32_t* black, int white, const uint32_t* bitmap, int64_t* out, void* ws, size_t ws_bytes,
                                       void* stream) {
    if ((p != 2 && p != 6) || F < 0 || F > 65535 || Hm < 0 || Wm < 0 || Hc < 0 || Hc > Hm || Wc < 0 || Wc > Wm || G < 1 || G > 4) return ELD_EINVAL;
    if (stride < 1 || stride > p || p % stride != 0) return ELD_EINVAL;
    if ((uint64_t)Hm * (uint64_t)Wm >= (1ull << 31) || !cell_groups_ok(p, group, G, black, white)) return ELD_EINVAL;
    (void)ws;
    if (ws_bytes < eld_tile_noise_workspace_bytes(F, Hm, Wm)) return ELD_EWS;
    const int nty = tiles_along(Hc, stride), ntx = tiles_along(Wc, stride);
    if (F == 0 || nty == 0 || ntx == 0) return 0;
    if (!frames || ((uintptr_t)frames & 1u) || !out || ((uintptr_t)out & 7u) || ((uintptr_t)bitmap & 3u)) return ELD_EINVAL;
    NoiseTileArgs a;
    a.frames = frames; a.bitmap = bitmap; a.out = (long long*)out;
    a.Hm = Hm; a.Wm = Wm; a.Hc = Hc; a.Wc = Wc; a.G = G; a.white = white; a.wpr = bitmap_pitch(Wm); a.ntx = ntx; a.nty = nty;
    a.hw = (uint32_t)Hm * (uint32_t)Wm;
    a.total = (unsigned long long)F * a.hw;
    a.dntx = make_fastdiv((uint32_t)ntx);
    a.counted = 0;
    for (int k = 0; k < 36; ++k) a.tab[k] = 0;
    for (int cy = 0; cy < p; ++cy)
        for (int cx = 0; cx < p; ++cx) {
            const int c = cy * p + cx, g = group[c];
            if (g >= 0) a.counted |= 1ull << c;
            bool same = g >= 0;
            int b9 = 0;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int n = ((cy + dy * stride + p) % p) * p + (cx + dx * stride + p) % p;
                    same = same && group[n] == g;
                    b9 += black[n];
                }
            a.tab[c] = b9 | ((same ? g + 1 : 0) << 24);         // b9 <= 9 * 65535 < 2^20
        }
    const bool vec = !((uintptr_t)frames & 15u);
    const dim3 grid((unsigned)(nty * ntx), (unsigned)F);        // nty * ntx <= Hm * Wm / 256 < 2^23
    hipStream_t s = as_stream(stream);
    if (p == 2) return stride == 1 ? launch_noise_tiles<2, 1>(a, vec, grid, s) : launch_noise_tiles<2, 2>(a, vec, grid, s);
    switch (stride) {
        case 1: return launch_noise_tiles<6, 1>(a, vec, grid, s);
        case 2: return launch_noise_tiles<6, 2>(a, vec, grid, s);
        case 3: return launch_noise_tiles<6, 3>(a, vec, grid, s);
        default: return launch_noise_tiles<6, 6>(a, vec, grid, s);
    }
}
