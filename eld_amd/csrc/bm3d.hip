// bm3d.hip -- BM3D over the packed planes of a variance-stabilised frame, grouped across the CFA planes: the classical baseline the paper's
// tables open with (eld_amd/classical.py).
//
//   eld_bm3d_vst_f32     float32 planes [N][C][h][w] of codes / qscale -> stabilised codes through a per-plane table -> block matching shared by
//                        the planes, a Walsh-Hadamard transform over [planes][group][8][8], hard thresholding (step 1) or an empirical Wiener
//                        filter guided by step 1's output (step 2), windowed aggregation; int32 in units of 2^-frac of a stabilised code
// Integer arithmetic from the table lookup on, and the aggregation is integer addition: the output depends neither on the launch geometry nor
// on the order of the atomic adds, and tests/bm3d_ref.py restates the contract of include/eld_amd.h in NumPy, bit for bit.
//
// Three launches behind one memset of the accumulators:
//   codes     x -> v, 16-bit codes in the workspace (one table lookup per site instead of one per site and overlapping search window)
//   blocks    one workgroup of 256 threads per reference block, below
//   quotient  out = (2 num + den) / (2 den), one 64-bit division per site and plane
// A reference block's workgroup
//   stages    the guide codes of its search window, (2S + 8)^2 sites of every plane, in LDS (0 outside the plane: never read by a candidate
//             that counts), eight loads in flight per thread;
//   matches   a thread takes the candidates k = tid, tid + 256, ... (at most 5) and keeps their distances in registers: 64 C clamped squared
//             differences each, a row of the reference block read once for all of them; the 41-bit keys go to LDS.  A box sum of the
//             per-position difference, as csrc/nlm.hip forms it, would share differences between the reference blocks of a tile, but only
//             every step-th box sum of a row is wanted, so the running sums NLM gets per site do not carry over: at step 3 the sharing is
//             64 / 9 at best against three more barriers per offset.  Not done; DESIGN.md sec. 25 has what matching costs as it is.
//   selects   G rounds of a wave-wide minimum over the keys, each the least key above the one before (keys are unique), so nothing is
//             written between the rounds and every wave finds the same list without a barrier; no sort.  The low bits of a key are 0 for
//             d = 0 and 1 + the offset's index otherwise, so the reference block leads its group even among exact duplicates;
//   transforms  the [M][G][8][8] array is one vector of 2^(lm + lg + 6) values whose index bits are the four axes, and the four-axis
//             Sylvester transform is the plain fast Walsh-Hadamard transform over all index bits: radix-4 passes in LDS, one barrier each,
//             four quads read before any is written;
//   shrinks   step 1: |T| > par[lg];  step 2: R = floor(4096 E / (E + par[lg])) from the transform of the guide blocks (kept as 16 bits),
//             the quotient from a float estimate corrected by 64-bit products;
//   inverts   the same transform again, and adds W win[u] est into the 64-bit numerators and W win[u] into the denominators with global
//             atomics: G 64 (M + 1) adds per set, 8 rows of 64 contiguous bytes per wave instruction.
// One wave per reference block (the first version) left six waves on a CU -- the LDS of a Bayer block is 24.7 KB -- and ran at the latency of
// its own LDS and memory accesses: 39 / 60 ms for the two steps of a 4 x 1424 x 2128 frame against 25 / 31 ms with four waves per block.
//
// Widths.  Codes <= 32767 and at most 2^14 values in a set: every partial sum of the forward transform is at most 32767 * 2^14 < 2^29.  After
// shrinkage |T'| <= |T|, but the partial sums of the INVERSE are bounded by sum |T'| only, which reaches 2^36 on adversarial input (Parseval:
// sum |T| <= L sqrt(L) 32767).  The workgroup sums |T'| first: below 2^31 -- every real frame -- the inverse runs in 32 bits, exactly; otherwise each
// output is summed by its definition in 64 bits (L^2 operations, no further LDS), so the contract holds for every input.
// The ratio R: E < 2^58, so E << 12 needs 70 bits; floor(4096 E / (E + p)) = 4096 - ceil(4096 p / (E + p)) needs 44 over 59.
// T R + 2048 < 2^43.  W <= 2^20, win <= 16, est < 2^19: one contribution < 2^43; the header's count of contributions gives num < 2^58, den < 2^39.
// W >= 2^20 / 2^14 (step 1) and 2^44 / (2^24 2^14) (step 2): at least 64, and every site lies under a reference block, so den >= 64.
#include "mosaic_dev.h"

namespace {

constexpr int BM_MAX_S = 16, BM_MAX_C = 16, BM_MAX_STEP = 8, BM_MAX_FRAC = 4;
constexpr int BM_BATCH = 4;                        // quads of a transform pass a lane reads before it writes: LDS latency once per batch
constexpr int BM_THREADS = 256, BM_WAVES = BM_THREADS / ELD_WAVE;      // a workgroup: one reference block
constexpr int BM_KPL = 5;                          // candidates per thread at most: ceil(33^2 / 256)
constexpr int BM_LOADS = 8;                        // global loads a lane has in flight while it stages
constexpr size_t BM_LDS_MAX = 152 * 1024;          // >= bm3d_lds(16, 16, 16, 16, true).total = 149664

struct Bm3dArgs {
    const int16_t* v;
    const int32_t* guide;
    unsigned long long* num;
    unsigned long long* den;
    int C, h, w, S, step, Gmax, mix, frac, ny, nx, nfy, nfx;
    uint32_t tau;
    uint32_t par[5];
    uint8_t win[64];
    FastDiv div_ww, div_side, div_ps;
};

struct Bm3dLds {
    size_t big, rb, grp, total;                     // byte offsets of the transform / key buffer, the ratios, the group list; the size
};

__host__ __device__ inline Bm3dLds bm3d_lds(int C, int S, int M, int Gmax, bool wiener) {
    const size_t WW = 2 * S + 8, side = 2 * S + 1, L = (size_t)M * Gmax * 64;
    Bm3dLds l;
    l.big = (C * WW * WW * 2 + 7) & ~(size_t)7;
    size_t big = L * 4 > side * side * 8 ? L * 4 : side * side * 8;
    big = (big + 7) & ~(size_t)7;
    l.rb = l.big + big;
    l.grp = l.rb + (wiener ? L * 2 : 0);
    l.total = l.grp + 16 * sizeof(int) + BM_WAVES * sizeof(unsigned long long) + 64;      // the group, the partial sums, the window table
    return l;
}

__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const unsigned long long t = __shfl_xor(v, o, 64);
        v = t < v ? t : v;
    }
    return v;
}

// the unnormalised Walsh-Hadamard transform over all nb index bits of T[0 .. 2^nb), in place; nb >= 6; ends behind a barrier
__device__ __forceinline__ void bm3d_wht(int32_t* T, int nb, int tid) {
    const int L = 1 << nb;
    int s = 0;
    for (; s + 1 < nb; s += 2) {
        const int low = (1 << s) - 1, st = 1 << s;
        for (int q0 = tid; q0 < (L >> 2); q0 += BM_BATCH * BM_THREADS) {                                  // BM_BATCH quads read before any is written
            int32_t r[BM_BATCH][4];
            int i0[BM_BATCH];
#pragma unroll
            for (int j = 0; j < BM_BATCH; ++j) {
                const int q = q0 + j * BM_THREADS;
                i0[j] = q < (L >> 2) ? (((q >> s) << (s + 2)) | (q & low)) : -1;
                if (i0[j] >= 0) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) r[j][e] = T[i0[j] + e * st];
                }
            }
#pragma unroll
            for (int j = 0; j < BM_BATCH; ++j) {
                if (i0[j] >= 0) {
                    const int32_t ab = r[j][0] + r[j][1], amb = r[j][0] - r[j][1], cd = r[j][2] + r[j][3], cmd = r[j][2] - r[j][3];
                    T[i0[j]] = ab + cd;
                    T[i0[j] + st] = amb + cmd;
                    T[i0[j] + 2 * st] = ab - cd;
                    T[i0[j] + 3 * st] = amb - cmd;
                }
            }
        }
        __syncthreads();
    }
    if (s < nb) {
        const int low = (1 << s) - 1, st = 1 << s;
        for (int q = tid; q < (L >> 1); q += BM_THREADS) {
            const int i0 = ((q >> s) << (s + 1)) | (q & low);
            const int32_t a = T[i0], b = T[i0 + st];
            T[i0] = a + b;
            T[i0 + st] = a - b;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void bm3d_codes_kernel(const float* x, const uint16_t* fwd, int16_t* v, int C, size_t hw, size_t total, float qscale) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)((i / hw) % (size_t)C);
    const float f = fminf(fmaxf(rintf(x[i] * qscale), 0.f), 65535.f);                                  // fmaxf(NaN, 0) = 0
    const uint32_t t = fwd[(size_t)c * 65536 + (int)f];
    v[i] = (int16_t)(t < 32767u ? t : 32767u);
}

__global__ __launch_bounds__(256) void bm3d_quotient_kernel(const unsigned long long* num, const unsigned long long* den, int32_t* out, int C, int mix,
                                                            size_t hw, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const size_t plane = i / hw, site = i - plane * hw;                                                  // plane = n C + c
    const unsigned long long d = den[(mix ? plane / (size_t)C : plane) * hw + site];
    out[i] = d ? (int32_t)((2ull * num[i] + d) / (2ull * d)) : 0;                                        // d >= 64 (above)
}

// the sum of v over the workgroup, the same in every thread; red: BM_WAVES values in LDS; two barriers
__device__ __forceinline__ unsigned long long block_sum(unsigned long long v, unsigned long long* red, int tid) {
    v = wave_sum(v);
    __syncthreads();                                                                                     // the last sum has been read
    if ((tid & (ELD_WAVE - 1)) == 0) red[tid >> 6] = v;
    __syncthreads();
    unsigned long long t = 0;
#pragma unroll
    for (int k = 0; k < BM_WAVES; ++k) t += red[k];
    return t;
}

template <bool WIENER>
__global__ __launch_bounds__(BM_THREADS) void bm3d_block_kernel(Bm3dArgs a) {
    extern __shared__ __align__(16) unsigned char bm_smem[];
    const int tid = threadIdx.x, lane = tid & (ELD_WAVE - 1);
    const int C = a.C, S = a.S, h = a.h, w = a.w;
    const int WW = 2 * S + 8, PS = WW * WW, side = 2 * S + 1, ncand = side * side, centre = S * side + S;
    const int M = a.mix ? C : 1, lm = 31 - __clz(M), nsets = a.mix ? 1 : C;
    const Bm3dLds lds = bm3d_lds(C, S, M, a.Gmax, WIENER);
    int16_t* gw = reinterpret_cast<int16_t*>(bm_smem);
    int32_t* T = reinterpret_cast<int32_t*>(bm_smem + lds.big);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(bm_smem + lds.big);              // until the group is chosen
    uint16_t* Rb = reinterpret_cast<uint16_t*>(bm_smem + lds.rb);
    int* grp = reinterpret_cast<int*>(bm_smem + lds.grp);                                              // (dy + S) << 8 | (dx + S), key order
    unsigned long long* red = reinterpret_cast<unsigned long long*>(grp + 16);
    uint8_t* wl = reinterpret_cast<uint8_t*>(red + BM_WAVES);

    const unsigned b = blockIdx.x;
    const int bx = (int)(b % (unsigned)a.nx), by = (int)((b / (unsigned)a.nx) % (unsigned)a.ny), n = (int)(b / ((unsigned)a.nx * (unsigned)a.ny));
    const int py = by < a.nfy ? by * a.step : h - 8, px = bx < a.nfx ? bx * a.step : w - 8;       // the last row / column of corners ends at the edge
    const size_t hw = (size_t)h * w;
    if (tid < 64) wl[tid] = a.win[tid];

    // ---- stage the guide codes of the search window ---------------------------------------------------------------------------------------------
    // BM_LOADS loads are issued before the first is used
    const int staged = C * PS;
    for (int i0 = tid; i0 < staged; i0 += BM_LOADS * BM_THREADS) {
        int raw[BM_LOADS];
#pragma unroll
        for (int j = 0; j < BM_LOADS; ++j) {
            const int i = i0 + j * BM_THREADS;
            raw[j] = 0;
            if (i < staged) {
                const int c = (int)fdiv_u32((uint32_t)i, a.div_ps), k = i - c * PS;
                const int wy = (int)fdiv_u32((uint32_t)k, a.div_ww), wx = k - wy * WW;
                const int gy = py - S + wy, gx = px - S + wx;
                if (gy >= 0 && gy < h && gx >= 0 && gx < w) {
                    const size_t at = ((size_t)n * C + c) * hw + (size_t)gy * w + gx;
                    raw[j] = WIENER ? a.guide[at] : (int)a.v[at];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < BM_LOADS; ++j) {
            const int i = i0 + j * BM_THREADS;
            if (i < staged) {
                int g = raw[j];
                if (WIENER) {                                                                            // outside the plane: 0 stays 0
                    const long long t = ((long long)g + ((1 << a.frac) >> 1)) >> a.frac;
                    g = (int)(t < 0 ? 0 : t > 32767 ? 32767 : t);
                }
                gw[i] = (int16_t)g;
            }
        }
    }
    __syncthreads();

    // ---- block distances and keys --------------------------------------------------------------------------------------------------------------
    // A thread owns the candidates k = tid + 256 j.  Plane by plane and row by row the reference block's 8 codes are read once (a broadcast) and
    // used for all of the thread's candidates: per difference one LDS read, not two.  A slot beyond the last candidate repeats the last one and
    // a candidate that leaves the plane is summed like any other (the window holds zeros there); neither gets a key.
    uint32_t D[BM_KPL];
    int boff[BM_KPL];
#pragma unroll
    for (int j = 0; j < BM_KPL; ++j) {
        const int k = min(tid + j * BM_THREADS, ncand - 1);
        const int dyi = (int)fdiv_u32((uint32_t)k, a.div_side);
        boff[j] = dyi * WW + (k - dyi * side);                                                           // rows dyi .. dyi + 7 <= 2S + 7 = WW - 1
        D[j] = 0u;
    }
    for (int c = 0; c < C; ++c) {
        for (int y = 0; y < 8; ++y) {
            const int16_t* Ar = gw + c * PS + (S + y) * WW + S;
            const int16_t* Br = gw + c * PS + y * WW;
            int A[8];
#pragma unroll
            for (int x = 0; x < 8; ++x) A[x] = Ar[x];
#pragma unroll
            for (int j = 0; j < BM_KPL; ++j) {
                if (j * BM_THREADS + (tid & ~(ELD_WAVE - 1)) < ncand) {                                  // wave-uniform
#pragma unroll
                    for (int x = 0; x < 8; ++x) {
                        const int df = min(max(A[x] - (int)Br[boff[j] + x], -1023), 1023);
                        D[j] += (uint32_t)__mul24(df, df);                                               // <= 1023^2 * 64 * 16 < 2^30
                    }
                }
            }
        }
    }
    unsigned long long counted = 0;
#pragma unroll
    for (int j = 0; j < BM_KPL; ++j) {
        const int k = tid + j * BM_THREADS;
        if (k < ncand) {
            const int dyi = (int)fdiv_u32((uint32_t)k, a.div_side), dxi = k - dyi * side;
            const int qy = py + dyi - S, qx = px + dxi - S;
            unsigned long long key = ~0ull;
            if (qy >= 0 && qy <= h - 8 && qx >= 0 && qx <= w - 8 && D[j] <= a.tau) {                     // the whole block inside the plane
                key = ((unsigned long long)D[j] << 11) | (unsigned)(k == centre ? 0 : k + 1);            // the reference block leads its group
                ++counted;
            }
            keys[k] = key;
        }
    }
    counted = block_sum(counted, red, tid);                                                              // >= 1: d = 0 has D = 0; the keys are visible
    const int nsel = (int)(counted < (unsigned long long)a.Gmax ? counted : (unsigned long long)a.Gmax);
    const int lg = nsel > 0 ? 31 - __clz(nsel) : 0, G = 1 << lg;
    // Every wave picks the same G keys, each the least above the one before (keys are unique; the reference block's is 0): nothing is written
    // between the rounds, so they need no barrier.
    {
        unsigned long long prev = 0;
        for (int r = 0; r < G; ++r) {
            unsigned long long best = ~0ull;
            for (int k = lane; k < ncand; k += ELD_WAVE) {
                const unsigned long long key = keys[k];
                best = ((r == 0 || key > prev) && key < best) ? key : best;
            }
            best = wave_min(best);
            prev = best;
            const int rk = best == ~0ull ? 0 : (int)(best & 2047u);                                      // G <= counted: a key is always left
            const int kk = rk ? rk - 1 : centre;
            if (tid == 0) {
                const int dyi = (int)fdiv_u32((uint32_t)kk, a.div_side);
                grp[r] = (dyi << 8) | (kk - dyi * side);
            }
        }
    }
    __syncthreads();                                                                                     // the group is known, the keys are done with

    // ---- per set of planes: transform, shrink, invert, aggregate ----------------------------------------------------------------------------------
    const int nb = 6 + lg + lm, L = 1 << nb, sh = nb - a.frac;                                           // sh >= 2
    const uint32_t p = a.par[lg];
    const long long est_max = (long long)32767 << a.frac;
    for (int s = 0; s < nsets; ++s) {
        unsigned long long sum_abs = 0, W;
        if (WIENER) {
            for (int i = tid; i < L; i += BM_THREADS) {
                const int mg = i >> 6, c = s * M + (mg >> lg), e = grp[mg & (G - 1)];
                T[i] = gw[c * PS + ((e >> 8) + ((i >> 3) & 7)) * WW + (e & 255) + (i & 7)];
            }
            __syncthreads();
            bm3d_wht(T, nb, tid);
            unsigned long long sum_r2 = 0;
            for (int i = tid; i < L; i += BM_THREADS) {
                const long long t = T[i];
                const unsigned long long den = (unsigned long long)(t * t) + p, nume = (unsigned long long)p << 12;
                uint32_t R = 4095u;                                                                      // den > nume: the ceiling is 1 (p >= 1)
                if (den <= nume) {
                    uint32_t q = (uint32_t)((float)nume / (float)den);                                   // <= 4096: within 1 of the quotient
                    while ((unsigned long long)q * den > nume) --q;
                    while ((unsigned long long)(q + 1u) * den <= nume) ++q;
                    R = 4096u - (q + ((unsigned long long)q * den != nume));
                }
                Rb[i] = (uint16_t)R;
                sum_r2 += (unsigned long long)R * R;
            }
            sum_r2 = block_sum(sum_r2, red, tid);                                                        // its barriers: T has been read
            W = (1ull << 44) / (sum_r2 > (1ull << 24) ? sum_r2 : (1ull << 24));
            for (int i0 = tid; i0 < L; i0 += BM_LOADS * BM_THREADS) {                                    // v is not the staged guide: from memory
                int raw[BM_LOADS];
#pragma unroll
                for (int j = 0; j < BM_LOADS; ++j) {
                    const int i = i0 + j * BM_THREADS;
                    raw[j] = 0;
                    if (i < L) {
                        const int mg = i >> 6, c = s * M + (mg >> lg), e = grp[mg & (G - 1)];
                        raw[j] = a.v[((size_t)n * C + c) * hw + (size_t)(py + (e >> 8) - S + ((i >> 3) & 7)) * w + (px + (e & 255) - S + (i & 7))];
                    }
                }
#pragma unroll
                for (int j = 0; j < BM_LOADS; ++j) {
                    const int i = i0 + j * BM_THREADS;
                    if (i < L) T[i] = raw[j];
                }
            }
        } else {
            for (int i = tid; i < L; i += BM_THREADS) {
                const int mg = i >> 6, c = s * M + (mg >> lg), e = grp[mg & (G - 1)];
                T[i] = gw[c * PS + ((e >> 8) + ((i >> 3) & 7)) * WW + (e & 255) + (i & 7)];
            }
        }
        __syncthreads();
        bm3d_wht(T, nb, tid);
        if (WIENER) {
            for (int i = tid; i < L; i += BM_THREADS) {
                const int32_t t = (int32_t)(((long long)T[i] * (long long)Rb[i] + 2048) >> 12);
                T[i] = t;
                sum_abs += (unsigned long long)(t < 0 ? -(long long)t : (long long)t);
            }
        } else {
            unsigned long long nnz = 0;
            for (int i = tid; i < L; i += BM_THREADS) {
                const int32_t t = T[i];
                const uint32_t m = (uint32_t)(t < 0 ? -t : t);
                if (m > p) {
                    ++nnz;
                    sum_abs += m;
                } else {
                    T[i] = 0;
                }
            }
            nnz = block_sum(nnz, red, tid);
            W = (1ull << 20) / (nnz > 1 ? nnz : 1);
        }
        sum_abs = block_sum(sum_abs, red, tid);                                                          // its barriers: T' is visible
        const bool narrow = sum_abs < (1ull << 31);                                                      // the same in every thread
        if (narrow) bm3d_wht(T, nb, tid);
        for (int i = tid; i < L; i += BM_THREADS) {
            long long I;
            if (narrow) {
                I = T[i];
            } else {
                I = 0;
                for (int k = 0; k < L; ++k) {
                    const long long t = T[k];
                    I += (__popc((unsigned)(i & k)) & 1) ? -t : t;
                }
            }
            long long est = (I + (1ll << (sh - 1))) >> sh;
            est = est < 0 ? 0 : est > est_max ? est_max : est;
            const int mg = i >> 6, m = mg >> lg, e = grp[mg & (G - 1)];
            const size_t site = (size_t)(py + (e >> 8) - S + ((i >> 3) & 7)) * w + (px + (e & 255) - S + (i & 7));
            const unsigned long long wu = W * (unsigned long long)wl[i & 63];
            atomicAdd(a.num + ((size_t)n * C + s * M + m) * hw + site, wu * (unsigned long long)est);
            if (m == 0) atomicAdd(a.den + ((size_t)n * nsets + s) * hw + site, wu);
        }
        __syncthreads();                                                                                 // the next set overwrites T
    }
}

template <bool WIENER>
int bm3d_launch(const Bm3dArgs& a, unsigned blocks, size_t lds, hipStream_t st) {
    static EldAttrOnce once;
    const int rc = once.ensure(bm3d_block_kernel<WIENER>, BM_LDS_MAX);
    if (rc) return rc;
    ELD_LAUNCH(bm3d_block_kernel<WIENER>, dim3(blocks), dim3(BM_THREADS), lds, st, a);
    ELD_LAUNCH_CHECK();
    return 0;
}

bool bm3d_shape_ok(int N, int C, int h, int w) { return N >= 1 && C >= 1 && C <= BM_MAX_C && h >= 8 && w >= 8; }

}  // namespace

// [num: N C h w u64][den: N C h w u64, the first N * sets planes used][v: N C h w i16]
extern "C" size_t eld_bm3d_vst_workspace_bytes(int N, int C, int h, int w) {
    if (!bm3d_shape_ok(N, C, h, w)) return 0;
    const size_t total = (size_t)N * C * h * w;
    return (total * 18 + 7) & ~(size_t)7;
}

extern "C" int eld_bm3d_vst_f32(const float* x, int N, int C, int h, int w, float qscale, const uint16_t* fwd, const int32_t* guide, int S, int step,
                                int Gmax, int mix, uint32_t tau, const uint32_t* par, const uint8_t* win, int frac, int32_t* out, void* ws,
                                size_t ws_bytes, void* stream) {
    if (!bm3d_shape_ok(N, C, h, w) || S < 0 || S > BM_MAX_S || step < 1 || step > BM_MAX_STEP || frac < 0 || frac > BM_MAX_FRAC) return ELD_EINVAL;
    if (Gmax != 1 && Gmax != 2 && Gmax != 4 && Gmax != 8 && Gmax != 16) return ELD_EINVAL;
    if ((mix != 0 && mix != 1) || (mix && (C & (C - 1))) || tau >= (1u << 30)) return ELD_EINVAL;
    if (!x || !fwd || !par || !win || !out || !ws) return ELD_EINVAL;
    if (((uintptr_t)x & 3u) || ((uintptr_t)fwd & 1u) || ((uintptr_t)out & 3u) || ((uintptr_t)guide & 3u) || ((uintptr_t)ws & 7u)) return ELD_EINVAL;
    for (int k = 0; k < 64; ++k)
        if (win[k] < 1 || win[k] > 16) return ELD_EINVAL;
    if (guide)
        for (int k = 0; k < 5; ++k)
            if (par[k] < 1) return ELD_EINVAL;
    const size_t hw = (size_t)h * w, total = (size_t)N * C * hw;
    const int nfy = (h - 8) / step + 1, nfx = (w - 8) / step + 1;
    const int ny = nfy + ((h - 8) % step != 0), nx = nfx + ((w - 8) % step != 0);
    const unsigned long long blocks = (unsigned long long)ny * nx * N;
    if (blocks > 0x7FFFFFFFull || (total + 255) / 256 > 0x7FFFFFFFull) return ELD_EINVAL;
    if (ws_bytes < eld_bm3d_vst_workspace_bytes(N, C, h, w)) return ELD_EWS;

    Bm3dArgs a;
    a.num = reinterpret_cast<unsigned long long*>(ws);
    a.den = a.num + total;
    int16_t* v = reinterpret_cast<int16_t*>(a.den + total);
    a.v = v; a.guide = guide;
    a.C = C; a.h = h; a.w = w; a.S = S; a.step = step; a.Gmax = Gmax; a.mix = mix; a.frac = frac;
    a.ny = ny; a.nx = nx; a.nfy = nfy; a.nfx = nfx; a.tau = tau;
    for (int k = 0; k < 5; ++k) a.par[k] = par[k];
    for (int k = 0; k < 64; ++k) a.win[k] = win[k];
    a.div_ww = make_fastdiv((uint32_t)(2 * S + 8));
    a.div_side = make_fastdiv((uint32_t)(2 * S + 1));
    a.div_ps = make_fastdiv((uint32_t)((2 * S + 8) * (2 * S + 8)));
    const hipStream_t st = as_stream(stream);
    const size_t lds = bm3d_lds(C, S, mix ? C : 1, Gmax, guide != nullptr).total;                        // at most 149664 of the 160 KB
    const hipError_t e = hipMemsetAsync(ws, 0, total * 16, st);                                          // the entry clears what it accumulates into
    if (e != hipSuccess) return (int)e;
    const unsigned eb = (unsigned)((total + 255) / 256);
    ELD_LAUNCH(bm3d_codes_kernel, dim3(eb), dim3(256), 0, st, x, fwd, v, C, hw, total, qscale);
    ELD_LAUNCH_CHECK();
    const int rc = guide ? bm3d_launch<true>(a, (unsigned)blocks, lds, st) : bm3d_launch<false>(a, (unsigned)blocks, lds, st);
    if (rc) return rc;
    ELD_LAUNCH(bm3d_quotient_kernel, dim3(eb), dim3(256), 0, st, (const unsigned long long*)a.num, (const unsigned long long*)a.den, out, C, mix, hw,
               total);
    ELD_LAUNCH_CHECK();
    return 0;
}
