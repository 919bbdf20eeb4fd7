// The fast guide tree of align_from_structure_files (multiple_alignment.py:496-508, full=False): shapemer index lists
// -> count matrix (make_count_matrix, :130-136 / :390-396) -> all-vs-all Bray-Curtis distances (braycurtis, :139-145).
// Included at the end of cr_api.hip.
//
// Numerics: the counts are non-negative integers, so both sums of braycurtis are exact integers in any order.  Here
// they are u32 sums on the device (numerator sum_k |a_k - b_k|, denominator n_a + n_b, both < 2^32 because every row
// sum is kept below 2^31), and the one f64 division of the epilogue is HIP's correctly rounded `/` on double
// (v_div_scale / v_div_fmas / v_div_fixup).  The result is the reference's bit for bit, 0.0 on the diagonal included.
//
// Layout: the counts of a side live in one u32 matrix of sh_rows_pad(rows) x sh_bins_pad(K) (zero padded; the padding
// adds |0 - 0| = 0).  The distance kernel reads them packed into 32-bit words: 4 bins per word (u8, every count
// <= 255), 2 (u16, <= 65 535) or 1 (u32); the packing is chosen from the largest count the count kernel measured.
#pragma once

namespace cr {

constexpr int kShTile = 64;            // proteins per tile side (Ti = Tj)
constexpr int kShThreads = 256;        // 16 x 16 lanes, each with a 4 x 4 block of accumulators
constexpr int kShChunkWords = 32;      // packed words per row streamed through LDS per step
constexpr int kShLdsStride = kShChunkWords + 4;    // 16-B padding: the 16 column rows of a lane group hit disjoint banks
constexpr int kShLdsBins = 8192;       // the count kernel's histogram lives in LDS up to this alphabet size (32 KiB)

// packing forms (CARETTA_SHAPEMER_FORM forces one that can hold the counts; 0: the library's choice).  A u16 form on
// v_sad_u16 (one per half word, the high half shifted down) was measured slower than kShU16Min (5.5 against 4.7 ms at
// P = 16 384) and WRONG on MI355X: its sums came out 1.50 x the true ones, as if v_sad_u16 summed both halves of its
// operands; it is not built.
enum ShForm { kShAuto = 0, kShU8Sad = 1, kShU16Min = 2, kShU32Sad = 3 };

inline int64_t sh_rows_pad(int64_t rows) { return (rows + kShTile - 1) / kShTile * kShTile; }
// bins per row of the u32 count matrix: a whole number of LDS chunks in every packing (4 bins per word at most)
inline int64_t sh_bins_pad(int64_t k) { return (k + 4 * kShChunkWords - 1) / (4 * kShChunkWords) * (4 * kShChunkWords); }

__device__ inline void sh_block_stats(uint32_t row_max, uint32_t* s_max, uint32_t* stat) {
    // one LDS atomic per lane, one global atomic per workgroup
    atomicMax(s_max, row_max);
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(&stat[1], *s_max);
}

// One workgroup per protein: the histogram of its index list.  cnt: u32 (rows_pad x ks), zeroed by the caller, may be
// null when only f64 counts are wanted and K fits in LDS; f: f64 (P x K) or null.  stat[0] |= 1 on an index outside
// [0, K) (that index is not counted); stat[1] = max over all counts.
__global__ __launch_bounds__(kShThreads) void k_shapemer_counts(const int32_t* __restrict__ idx, const int64_t* __restrict__ off,
                                                               int k, int64_t ks, uint32_t* __restrict__ cnt,
                                                               double* __restrict__ f, uint32_t* __restrict__ n_out,
                                                               uint32_t* __restrict__ stat) {
    __shared__ uint32_t hist[kShLdsBins];
    __shared__ uint32_t s_max;
    const int64_t p = blockIdx.x;
    const int64_t beg = off[p], end = off[p + 1];
    const int t = threadIdx.x;
    const bool in_lds = k <= kShLdsBins;
    if (t == 0) s_max = 0;
    if (in_lds)
        for (int b = t; b < k; b += kShThreads) hist[b] = 0;
    __syncthreads();
    bool bad = false;
    uint32_t* row = cnt ? cnt + p * ks : nullptr;
    for (int64_t x = beg + t; x < end; x += kShThreads) {
        const int32_t v = idx[x];
        if (v < 0 || v >= k) {
            bad = true;
            continue;
        }
        if (in_lds) atomicAdd(&hist[v], 1u);
        else atomicAdd(&row[v], 1u);
    }
    if (bad) atomicOr(&stat[0], 1u);
    __syncthreads();
    uint32_t mx = 0;
    for (int b = t; b < k; b += kShThreads) {
        const uint32_t c = in_lds ? hist[b] : __hip_atomic_load(&row[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        mx = c > mx ? c : mx;
        if (in_lds && row) row[b] = c;
        if (f) f[p * k + b] = (double)c;
    }
    if (t == 0 && n_out) n_out[p] = (uint32_t)(end - beg);
    sh_block_stats(mx, &s_max, stat);
}

// braycurtis on caller counts: one workgroup per row turns f64 counts into u32.  A count that is negative, not an
// integer, NaN or above 2^31 - 1 sets stat[0] bit 2 (and counts as 0); a row sum above 2^31 - 1 sets bit 4; an empty
// row sets `empty_bit`.
__global__ __launch_bounds__(kShThreads) void k_counts_from_f64(const double* __restrict__ c, int k, int64_t ks,
                                                               uint32_t* __restrict__ cnt, uint32_t* __restrict__ n_out,
                                                               uint32_t* __restrict__ stat, uint32_t empty_bit) {
    __shared__ uint32_t s_max;
    __shared__ unsigned long long s_sum;
    const int64_t r = blockIdx.x;
    const int t = threadIdx.x;
    if (t == 0) {
        s_max = 0;
        s_sum = 0;
    }
    __syncthreads();
    uint32_t mx = 0;
    unsigned long long sum = 0;
    bool bad = false;
    for (int b = t; b < k; b += kShThreads) {
        const double v = c[r * k + b];
        const bool ok = v >= 0.0 && v <= 2147483647.0 && v == floor(v);     // NaN fails the first test
        const uint32_t u = ok ? (uint32_t)v : 0u;
        bad |= !ok;
        cnt[r * ks + b] = u;
        sum += u;
        mx = u > mx ? u : mx;
    }
    if (bad) atomicOr(&stat[0], 2u);
    atomicAdd(&s_sum, sum);
    __syncthreads();
    if (t == 0) {
        const unsigned long long total = s_sum;
        if (total > 2147483647ull) atomicOr(&stat[0], 4u);
        if (total == 0) atomicOr(&stat[0], empty_bit);
        n_out[r] = (uint32_t)(total > 2147483647ull ? 0 : total);
    }
    sh_block_stats(mx, &s_max, stat);
}

// u32 counts (stride ks bins) -> packed words (stride ks / bpw words), one thread per word, rows_pad rows
template <int BPW>
__global__ void k_pack_counts(const uint32_t* __restrict__ cnt, int64_t ks, int64_t words, uint32_t* __restrict__ out) {
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= words) return;
    const int64_t wpr = ks / BPW;
    const uint32_t* src = cnt + (x / wpr) * ks + (x % wpr) * BPW;
    uint32_t w = 0;
#pragma unroll
    for (int e = 0; e < BPW; e++) w |= src[e] << (e * (32 / BPW));
    out[x] = w;
}

// one packed word of a row against one of a column, added to the accumulator
template <int FORM>
__device__ inline uint32_t sh_word(uint32_t a, uint32_t b, uint32_t acc) {
    if constexpr (FORM == kShU8Sad) {
        return __builtin_amdgcn_sad_u8(a, b, acc);                          // 4 bins: sum |a_e - b_e|
    } else if constexpr (FORM == kShU16Min) {
        // |a - b| = a + b - 2 min(a, b): this form sums the minima, the epilogue forms n_a + n_b - 2 S
        typedef unsigned short us2 __attribute__((ext_vector_type(2)));
        const us2 m = __builtin_elementwise_min(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b));
        return __builtin_amdgcn_udot2(m, (us2){1, 1}, acc, false);
    } else {
        return acc + (a > b ? a - b : b - a);                               // v_sad_u32
    }
}

// All-vs-all L1 distances of two packed count matrices (words per row `w`, a multiple of kShChunkWords; rows padded to
// kShTile) in 64 x 64 tiles, VALU only.  sym: A == B, only the tiles on and above the diagonal run and each writes its
// mirror as well.  out: rows x cols f64, row-major.
template <int FORM>
__global__ __launch_bounds__(kShThreads) void k_braycurtis(const uint32_t* __restrict__ a, int64_t rows,
                                                          const uint32_t* __restrict__ b, int64_t cols, int64_t w,
                                                          const uint32_t* __restrict__ na, const uint32_t* __restrict__ nb,
                                                          int sym, double* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[2 * kShTile * kShLdsStride];
    static_assert(kShTile * (kShTile + 1) <= 2 * kShTile * kShLdsStride, "the result tile reuses the chunk buffers");
    uint32_t* sa = lds;
    uint32_t* sb = lds + kShTile * kShLdsStride;
    const int64_t ti = blockIdx.y, tj = blockIdx.x;
    if (sym && tj < ti) return;
    const int64_t i0 = ti * kShTile, j0 = tj * kShTile;
    const int t = threadIdx.x, tx = t % 16, ty = t / 16;
    const uint32_t* ga = a + i0 * w;
    const uint32_t* gb = b + j0 * w;
    uint32_t acc[4][4] = {};
    for (int64_t c0 = 0; c0 < w; c0 += kShChunkWords) {
        // 64 rows x 32 words per side: two 16-B pieces per thread per side
#pragma unroll
        for (int s = 0; s < 2; s++) {
            const int q = t + s * kShThreads, r = q / 8, c4 = (q % 8) * 4;
            const uint4 va = *reinterpret_cast<const uint4*>(ga + r * w + c0 + c4);
            const uint4 vb = *reinterpret_cast<const uint4*>(gb + r * w + c0 + c4);
            *reinterpret_cast<uint4*>(sa + r * kShLdsStride + c4) = va;
            *reinterpret_cast<uint4*>(sb + r * kShLdsStride + c4) = vb;
        }
        __syncthreads();
#pragma unroll 2
        for (int x = 0; x < kShChunkWords; x += 4) {
            uint4 ra[4], rb[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                ra[i] = *reinterpret_cast<const uint4*>(sa + (ty + 16 * i) * kShLdsStride + x);
                rb[i] = *reinterpret_cast<const uint4*>(sb + (tx + 16 * i) * kShLdsStride + x);
            }
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    acc[i][j] = sh_word<FORM>(ra[i].x, rb[j].x, acc[i][j]);
                    acc[i][j] = sh_word<FORM>(ra[i].y, rb[j].y, acc[i][j]);
                    acc[i][j] = sh_word<FORM>(ra[i].z, rb[j].z, acc[i][j]);
                    acc[i][j] = sh_word<FORM>(ra[i].w, rb[j].w, acc[i][j]);
                }
        }
        __syncthreads();
    }
    // the tile's sums through LDS, so that both the tile and its mirror are written with consecutive lanes on
    // consecutive columns
    uint32_t* st = lds;
    constexpr int kSt = kShTile + 1;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) st[(ty + 16 * i) * kSt + tx + 16 * j] = acc[i][j];
    __syncthreads();
    const bool mirror = sym && ti != tj;
    for (int e = t; e < kShTile * kShTile; e += kShThreads) {
        {
            const int r = e / kShTile, c = e % kShTile;
            const int64_t i = i0 + r, j = j0 + c;
            if (i < rows && j < cols) {
                const uint64_t den = (uint64_t)na[i] + nb[j];
                const uint64_t s = st[r * kSt + c];
                const uint64_t num = FORM == kShU16Min ? den - 2 * s : s;
                out[i * cols + j] = (double)num / (double)den;
            }
        }
        if (mirror) {
            const int c = e / kShTile, r = e % kShTile;        // out row j0 + c, column i0 + r
            const int64_t i = i0 + r, j = j0 + c;
            if (i < rows && j < cols) {
                const uint64_t den = (uint64_t)na[i] + nb[j];
                const uint64_t s = st[r * kSt + c];
                const uint64_t num = FORM == kShU16Min ? den - 2 * s : s;
                out[j * cols + i] = (double)num / (double)den;
            }
        }
    }
}

}  // namespace cr

namespace {

// u32 counts of one side on the device
struct ShSide {
    DevBuf<uint32_t> cnt, n, packed;
    int64_t rows = 0;
};

int sh_form_for(uint32_t max_count) {
    const int forced = g_cfg.shapemer_form;
    const uint32_t cap[4] = {0, 255u, 65535u, 0xffffffffu};
    if (forced >= cr::kShU8Sad && forced <= cr::kShU32Sad && max_count <= cap[forced]) return forced;
    return max_count <= 255u ? cr::kShU8Sad : max_count <= 65535u ? cr::kShU16Min : cr::kShU32Sad;
}

int sh_alloc_counts(ShSide& s, int64_t rows, int64_t k, cr_context* ctx) {
    s.rows = rows;
    const size_t n = (size_t)cr::sh_rows_pad(rows) * (size_t)cr::sh_bins_pad(k);
    CR_HIP(s.cnt.ensure(n));
    CR_HIP(hipMemsetAsync(s.cnt.p, 0, sizeof(uint32_t) * n, ctx->stream));
    CR_HIP(s.n.ensure((size_t)rows));
    return CR_OK;
}

int sh_stat_fetch(cr_context* ctx, const DevBuf<uint32_t>& stat, uint32_t out[2]) {
    return download(ctx, out, stat.p, 2 * sizeof(uint32_t));
}

// validated CSR lists -> u32 counts (and f64 counts when f != null) of one side
int sh_count_lists(cr_context* ctx, const int32_t* idx, const int64_t* offsets, int64_t p, int64_t k, ShSide* side,
                   double* f_dev, DevBuf<uint32_t>& stat) {
    const int64_t total = offsets[p];
    DevBuf<int32_t> didx;
    DevBuf<int64_t> doff;
    int rc = upload(doff, offsets, (size_t)p + 1, ctx);
    if (rc) return rc;
    if (total > 0 && (rc = upload(didx, idx, (size_t)total, ctx))) return rc;
    CR_LAUNCH(cr::k_shapemer_counts, dim3((unsigned)p), dim3(cr::kShThreads), 0, ctx->stream, didx.p, doff.p, (int)k,
              cr::sh_bins_pad(k), side ? side->cnt.p : nullptr, f_dev, side ? side->n.p : nullptr, stat.p);
    CR_HIP(hipGetLastError());
    return CR_OK;
}

int sh_check_lists(const int32_t* idx, const int64_t* offsets, int64_t p, int64_t k) {
    CR_REQUIRE(p >= 0 && p < (1ll << 31), "number of index lists out of range");
    CR_REQUIRE(k >= 1 && k <= (1ll << 24), "alphabet_size must be in [1, 2^24]");
    CR_REQUIRE(offsets != nullptr, "null offsets");
    CR_REQUIRE(offsets[0] == 0, "offsets[0] must be 0");
    for (int64_t i = 0; i < p; i++) {
        CR_REQUIRE(offsets[i + 1] >= offsets[i], "offsets must be non-decreasing");
        CR_REQUIRE(offsets[i + 1] - offsets[i] <= 2147483647ll, "an index list is longer than 2^31 - 1");
    }
    CR_REQUIRE(offsets[p] == 0 || idx != nullptr, "null indices");
    return CR_OK;
}

int sh_check_stat(uint32_t flags) {
    CR_REQUIRE(!(flags & 1u), "a shapemer index lies outside [0, alphabet_size)");
    CR_REQUIRE(!(flags & 2u), "counts must be non-negative integers below 2^31 (negative, non-integer or NaN count)");
    CR_REQUIRE(!(flags & 4u), "a row of counts sums to 2^31 or more");
    return CR_OK;
}

int sh_pack(cr_context* ctx, ShSide& s, int64_t k, int form) {
    if (form == cr::kShU32Sad) return CR_OK;
    const int bpw = form == cr::kShU8Sad ? 4 : 2;
    const int64_t words = cr::sh_rows_pad(s.rows) * cr::sh_bins_pad(k) / bpw;
    CR_HIP(s.packed.ensure((size_t)words));
    const dim3 grid((unsigned)((words + 255) / 256));
    if (bpw == 4) CR_LAUNCH(cr::k_pack_counts<4>, grid, dim3(256), 0, ctx->stream, s.cnt.p, cr::sh_bins_pad(k), words, s.packed.p);
    else CR_LAUNCH(cr::k_pack_counts<2>, grid, dim3(256), 0, ctx->stream, s.cnt.p, cr::sh_bins_pad(k), words, s.packed.p);
    CR_HIP(hipGetLastError());
    return CR_OK;
}

// the distance matrix of two counted sides (b == a: the symmetric case) into host `out` (a.rows x b.rows)
int sh_distances(cr_context* ctx, ShSide& a, ShSide& b, int64_t k, uint32_t max_count, double* out) {
    const bool sym = &a == &b;
    CR_REQUIRE(cr::sh_rows_pad(a.rows) / cr::kShTile <= 65535, "at most 4 194 240 rows on the first side");
    const int form = sh_form_for(max_count);
    int rc = sh_pack(ctx, a, k, form);
    if (!rc && !sym) rc = sh_pack(ctx, b, k, form);
    if (rc) return rc;
    const int64_t w = cr::sh_bins_pad(k) / (form == cr::kShU8Sad ? 4 : form == cr::kShU32Sad ? 1 : 2);
    const uint32_t* pa = form == cr::kShU32Sad ? a.cnt.p : a.packed.p;
    const uint32_t* pb = form == cr::kShU32Sad ? b.cnt.p : b.packed.p;
    DevBuf<double> dout;
    CR_HIP(dout.ensure((size_t)a.rows * (size_t)b.rows));
    const dim3 grid((unsigned)(cr::sh_rows_pad(b.rows) / cr::kShTile), (unsigned)(cr::sh_rows_pad(a.rows) / cr::kShTile));
    switch (form) {
        case cr::kShU8Sad: CR_LAUNCH(cr::k_braycurtis<cr::kShU8Sad>, grid, dim3(cr::kShThreads), 0, ctx->stream, pa, a.rows, pb, b.rows, w, a.n.p, b.n.p, (int)sym, dout.p); break;
        case cr::kShU16Min: CR_LAUNCH(cr::k_braycurtis<cr::kShU16Min>, grid, dim3(cr::kShThreads), 0, ctx->stream, pa, a.rows, pb, b.rows, w, a.n.p, b.n.p, (int)sym, dout.p); break;
        default: CR_LAUNCH(cr::k_braycurtis<cr::kShU32Sad>, grid, dim3(cr::kShThreads), 0, ctx->stream, pa, a.rows, pb, b.rows, w, a.n.p, b.n.p, (int)sym, dout.p); break;
    }
    CR_HIP(hipGetLastError());
    return download(ctx, out, dout.p, sizeof(double) * (size_t)a.rows * (size_t)b.rows);
}

}  // namespace

extern "C" {

int cr_count_matrix(cr_context* ctx, const int32_t* idx, const int64_t* offsets, int64_t num_lists, int64_t alphabet_size,
                    double* out) {
    int rc = set_device(ctx);
    if (rc || (rc = sh_check_lists(idx, offsets, num_lists, alphabet_size))) return rc;
    if (num_lists == 0) return CR_OK;
    CR_REQUIRE(out != nullptr, "null output");
    const int64_t k = alphabet_size;
    ShSide side;
    const bool need_u32 = k > cr::kShLdsBins;        // the global-atomic histogram needs the u32 rows
    if (need_u32 && (rc = sh_alloc_counts(side, num_lists, k, ctx))) return rc;
    DevBuf<double> f;
    DevBuf<uint32_t> stat;
    CR_HIP(f.ensure((size_t)num_lists * (size_t)k));
    CR_HIP(stat.ensure(2));
    CR_HIP(hipMemsetAsync(stat.p, 0, 2 * sizeof(uint32_t), ctx->stream));
    if ((rc = sh_count_lists(ctx, idx, offsets, num_lists, k, need_u32 ? &side : nullptr, f.p, stat))) return rc;
    uint32_t st[2];
    if ((rc = sh_stat_fetch(ctx, stat, st)) || (rc = sh_check_stat(st[0]))) return rc;
    return download(ctx, out, f.p, sizeof(double) * (size_t)num_lists * (size_t)k);
}

int cr_braycurtis(cr_context* ctx, const double* counts_1, int64_t p, const double* counts_2, int64_t m, int64_t k,
                  double* out) {
    int rc = set_device(ctx);
    if (rc) return rc;
    CR_REQUIRE(p >= 0 && m >= 0 && p < (1ll << 31) && m < (1ll << 31), "bad shape");
    CR_REQUIRE(k >= 1 && k <= (1ll << 24), "the count matrices need 1 to 2^24 columns");
    if (p == 0 || m == 0) return CR_OK;
    CR_REQUIRE(counts_1 && counts_2 && out, "null array");
    const bool sym = counts_1 == counts_2 && p == m;
    ShSide a, b;
    DevBuf<double> d1, d2;
    DevBuf<uint32_t> stat;
    CR_HIP(stat.ensure(2));
    CR_HIP(hipMemsetAsync(stat.p, 0, 2 * sizeof(uint32_t), ctx->stream));
    if ((rc = sh_alloc_counts(a, p, k, ctx)) || (rc = upload(d1, counts_1, (size_t)p * k, ctx))) return rc;
    CR_LAUNCH(cr::k_counts_from_f64, dim3((unsigned)p), dim3(cr::kShThreads), 0, ctx->stream, d1.p, (int)k,
              cr::sh_bins_pad(k), a.cnt.p, a.n.p, stat.p, 8u);
    CR_HIP(hipGetLastError());
    if (!sym) {
        if ((rc = sh_alloc_counts(b, m, k, ctx)) || (rc = upload(d2, counts_2, (size_t)m * k, ctx))) return rc;
        CR_LAUNCH(cr::k_counts_from_f64, dim3((unsigned)m), dim3(cr::kShThreads), 0, ctx->stream, d2.p, (int)k,
                  cr::sh_bins_pad(k), b.cnt.p, b.n.p, stat.p, 16u);
        CR_HIP(hipGetLastError());
    }
    uint32_t st[2];
    if ((rc = sh_stat_fetch(ctx, stat, st)) || (rc = sh_check_stat(st[0]))) return rc;
    // 0 / 0: an empty row of counts_1 against an empty row of counts_2 (in the symmetric case: any empty row, its
    // diagonal entry)
    CR_REQUIRE(!(sym ? (st[0] & 8u) : (st[0] & 8u) && (st[0] & 16u)),
               "both rows of a pair have no counts: Bray-Curtis distance 0 / 0 is undefined");
    return sh_distances(ctx, a, sym ? a : b, k, st[1], out);
}

int cr_shapemer_distance_matrix(cr_context* ctx, const int32_t* idx, const int64_t* offsets, int64_t num_lists,
                                int64_t alphabet_size, double* out) {
    int rc = set_device(ctx);
    if (rc || (rc = sh_check_lists(idx, offsets, num_lists, alphabet_size))) return rc;
    if (num_lists == 0) return CR_OK;
    CR_REQUIRE(out != nullptr, "null output");
    for (int64_t i = 0; i < num_lists; i++)
        CR_REQUIRE(offsets[i + 1] > offsets[i], "an empty index list: its Bray-Curtis distance to itself is 0 / 0");
    ShSide side;
    DevBuf<uint32_t> stat;
    CR_HIP(stat.ensure(2));
    CR_HIP(hipMemsetAsync(stat.p, 0, 2 * sizeof(uint32_t), ctx->stream));
    if ((rc = sh_alloc_counts(side, num_lists, alphabet_size, ctx))) return rc;
    if ((rc = sh_count_lists(ctx, idx, offsets, num_lists, alphabet_size, &side, nullptr, stat))) return rc;
    uint32_t st[2];
    if ((rc = sh_stat_fetch(ctx, stat, st)) || (rc = sh_check_stat(st[0]))) return rc;
    return sh_distances(ctx, side, side, alphabet_size, st[1], out);
}

}  // extern "C"
