// The structure-file front end of align_from_structure_files (multiple_alignment.py:399-593) and the all-atom moves of
// its PDB writers (write_superposed_pdbs_core / _references, :639-689, :786-853).  Included at the end of cr_api.hip,
// after cr_shapemer.h, whose count and distance kernels the fused guide-tree call feeds.
//
// Features.  The reference takes its per-residue tensors and shapemers from geometricus (moment invariants and the learned
// ShapemerLearn model, :479-488, :503-505), which is not available here.  The stand-in is helper.local_shape_descriptor:
// column b of residue i is the C-alpha distance to residue clip(i + o_b, 0, L - 1), o = -2, +2, -3, +3, ..., squashed
// with d / (d + 10).  The shapemer of a residue is its binarised row read as a w-bit number, first column most
// significant: the position of that 0/1 tuple in itertools.product([0, 1], repeat=w), the reference's key order (:503).
// Results from these features are NOT the reference's: they are outside the parity contract.
//
// Numerics: dist = sqrt((dx*dx + dy*dy) + dz*dz), numpy's order for np.linalg.norm(axis=1) on rows of 3; HIP's sqrt and
// `/` on double are correctly rounded and the library is built with -ffp-contract=off, so the tensors equal
// local_shape_descriptor's bit for bit.
#pragma once

namespace cr {

constexpr int kFtThreads = 256;
constexpr int kFtMaxWidth = 16;

// column b -> sequence offset of its neighbour: -2, +2, -3, +3, ...
CR_D int ft_offset(int b) {
    const int k = b / 2 + 2;
    return (b & 1) ? k : -k;
}

// One thread per output element, a workgroup covers whole rows (rows_per_block = kFtThreads / w), so the f64 stores of
// a workgroup are one contiguous run.  The rows' threshold bits meet in LDS, where one thread per row forms its index.
// off: P + 1 strictly increasing offsets from 0 (checked by the caller).  tensors may be null.
__global__ __launch_bounds__(kFtThreads) void k_structure_features(const double* __restrict__ x,
                                                                  const int64_t* __restrict__ off, int64_t P,
                                                                  int64_t total, int w, int rows_per_block,
                                                                  double* __restrict__ tensors,
                                                                  int32_t* __restrict__ idx) {
    __shared__ uint8_t bits[kFtThreads];
    const int t = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r = r0 + t / w;
    uint8_t bit = 0;
    if (t < rows_per_block * w && r < total) {
        int64_t lo = 0, hi = P;            // off[lo] <= r < off[hi]
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) / 2;
            if (off[mid] <= r) lo = mid;
            else hi = mid;
        }
        const int64_t beg = off[lo], len = off[lo + 1] - beg;
        int64_t j = r - beg + ft_offset(t % w);
        j = j < 0 ? 0 : (j > len - 1 ? len - 1 : j);
        const double* a = x + r * 3;
        const double* c = x + (beg + j) * 3;
        const double dx = a[0] - c[0], dy = a[1] - c[1], dz = a[2] - c[2];
        const double dist = sqrt((dx * dx + dy * dy) + dz * dz);
        const double v = dist / (dist + 10.0);
        if (tensors) tensors[r0 * w + t] = v;          // = row r, column t % w
        bit = v >= 0.5 ? 1 : 0;
    }
    bits[t] = bit;
    __syncthreads();
    if (t < rows_per_block && r0 + t < total) {
        int32_t code = 0;
        for (int b = 0; b < w; b++) code = (code << 1) | bits[t * w + b];
        idx[r0 + t] = code;
    }
}

// C-alpha rows of every structure out of its atoms: ca[off[s] + i] = atoms[aoff[s] + ca_row[off[s] + i]].  One wave per
// structure.
__global__ __launch_bounds__(kWave) void k_gather_calpha(const double* __restrict__ atoms, const int64_t* __restrict__ aoff,
                                                        const int64_t* __restrict__ off, const int32_t* __restrict__ ca_row,
                                                        double* __restrict__ ca) {
    const int s = blockIdx.x;
    for (int64_t r = off[s] + threadIdx.x; r < off[s + 1]; r += kWave) {
        const double* v = atoms + (aoff[s] + ca_row[r]) * 3;
        for (int a = 0; a < 3; a++) ca[r * 3 + a] = v[a];
    }
}

// k_core_superpose with a second array: the fit on the structure's C-alpha rows exactly as there, R and t applied to all
// of its atoms (write_superposed_pdbs_core, :639-689).  The reference structure is shifted by the core centroid.
__global__ __launch_bounds__(kWave) void k_core_superpose_atoms(const double* __restrict__ coords,
                                                               const int64_t* __restrict__ offsets,
                                                               const double* __restrict__ atoms,
                                                               const int64_t* __restrict__ aoff,
                                                               const int32_t* __restrict__ msa, int W,
                                                               const int32_t* __restrict__ core, int ncore, int ref,
                                                               const double* __restrict__ x1,
                                                               const double* __restrict__ centroid,
                                                               double* __restrict__ out) {
    extern __shared__ double lds[];
    const int lane = threadIdx.x, s = blockIdx.x;
    const double* X = coords + offsets[s] * 3;
    const int64_t n = aoff[s + 1] - aoff[s];
    const double* A = atoms + aoff[s] * 3;
    double* O = out + aoff[s] * 3;
    if (s == ref) {
        for (int64_t r = lane; r < n; r += kWave)
            for (int a = 0; a < 3; a++) O[r * 3 + a] = A[r * 3 + a] - centroid[a];
        return;
    }
    uint32_t* ent = reinterpret_cast<uint32_t*>(lds);
    double* scratch = lds + ((size_t)ncore + 3) / 4 * 2;
    for (int e = lane; e < ncore; e += kWave) ent[e] = pack_entry(e, msa[(int64_t)s * W + core[e]]);
    wave_sync();
    double c1[3], c2[3], Rm[9], t[3];
    kabsch_ordered(x1, X, ent, ncore, ncore, lane, scratch, c1, c2, Rm, t);
    for (int64_t r = lane; r < n; r += kWave) {
        const double v[3] = {A[r * 3], A[r * 3 + 1], A[r * 3 + 2]};
        double o[3];
        rot3(v, Rm, o);
        for (int a = 0; a < 3; a++) O[r * 3 + a] = o[a] + t[a];
    }
}

// k_reference_superpose with a second array: the structures listed in `which` fitted onto `ref_coords` over the columns
// they share with `ref`, R and t applied to all of their atoms (one group of write_superposed_pdbs_references,
// :786-853).  counts[b] = number of shared columns; a structure with 3 or fewer is left as it is (the caller rejects it).
__global__ __launch_bounds__(kWave) void k_reference_superpose_atoms(const double* __restrict__ coords,
                                                                    const int64_t* __restrict__ offsets,
                                                                    const double* __restrict__ atoms,
                                                                    const int64_t* __restrict__ aoff,
                                                                    const int32_t* __restrict__ msa, int W, int ref,
                                                                    const double* __restrict__ ref_coords,
                                                                    const int32_t* __restrict__ which,
                                                                    double* __restrict__ out, int32_t* __restrict__ counts) {
    extern __shared__ double lds[];
    const int lane = threadIdx.x, s = which[blockIdx.x];
    const double* X = coords + offsets[s] * 3;
    const int64_t n = aoff[s + 1] - aoff[s];
    const double* A = atoms + aoff[s] * 3;
    double* O = out + aoff[s] * 3;
    uint32_t* ent = reinterpret_cast<uint32_t*>(lds);
    double* scratch = lds + ((size_t)W + 3) / 4 * 2;
    int kloc = 0;
    for (int x = lane; x < W; x += kWave) {
        const int a = msa[(int64_t)ref * W + x], b = msa[(int64_t)s * W + x];
        const bool pair = a != -1 && b != -1;
        ent[x] = pair ? pack_entry(a, b) : pack_entry(-1, -1);
        kloc += pair ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) kloc += __shfl_xor(kloc, o);
    wave_sync();
    if (lane == 0) counts[blockIdx.x] = kloc;
    if (kloc <= 3) return;
    double c1[3], c2[3], Rm[9], t[3];
    kabsch_ordered(ref_coords, X, ent, W, kloc, lane, scratch, c1, c2, Rm, t);
    for (int64_t r = lane; r < n; r += kWave) {
        const double v[3] = {A[r * 3], A[r * 3 + 1], A[r * 3 + 2]};
        double o[3];
        rot3(v, Rm, o);
        for (int a = 0; a < 3; a++) O[r * 3 + a] = o[a] + t[a];
    }
}

}  // namespace cr

namespace {

int ft_check(const double* coords, const int64_t* offsets, int64_t p, int64_t w) {
    CR_REQUIRE(w >= 1 && w <= cr::kFtMaxWidth, "feature width must be in [1, 16]");
    CR_REQUIRE(p >= 1 && p < (1ll << 31), "number of structures out of range");
    CR_REQUIRE(offsets != nullptr, "null offsets");
    CR_REQUIRE(offsets[0] == 0, "offsets[0] must be 0");
    for (int64_t i = 0; i < p; i++) CR_REQUIRE(offsets[i + 1] > offsets[i], "an empty structure (offsets must increase)");
    CR_REQUIRE(offsets[p] <= 2147483647ll, "at most 2^31 - 1 residues in one call");
    CR_REQUIRE(coords != nullptr, "null coordinates");
    CR_REQUIRE(all_finite(coords, (size_t)offsets[p] * 3), "coordinates contain NaN or infinity");
    return CR_OK;
}

// checked inputs -> device tensors (when dt != null) and indices
int ft_run(cr_context* ctx, const double* coords, const int64_t* offsets, int64_t p, int64_t w, DevBuf<int64_t>& doff,
           DevBuf<double>* dt, DevBuf<int32_t>& didx) {
    const int64_t total = offsets[p];
    DevBuf<double> dc;
    int rc;
    if ((rc = upload(dc, coords, (size_t)total * 3, ctx)) || (rc = upload(doff, offsets, (size_t)p + 1, ctx))) return rc;
    if (dt) CR_HIP(dt->ensure((size_t)total * (size_t)w));
    CR_HIP(didx.ensure((size_t)total));
    const int rows = cr::kFtThreads / (int)w;
    CR_LAUNCH(cr::k_structure_features, dim3((unsigned)((total + rows - 1) / rows)), dim3(cr::kFtThreads), 0, ctx->stream,
              dc.p, doff.p, p, total, (int)w, rows, dt ? dt->p : nullptr, didx.p);
    CR_HIP(hipGetLastError());
    return CR_OK;
}

// atoms (aoff[p] rows) with a C-alpha row map per residue -> checked, uploaded, and the C-alpha rows gathered on the device
int ft_atoms_upload(cr_context* ctx, const double* atoms, const int64_t* aoff, const int32_t* ca_rows, const int64_t* offsets,
                    int64_t p, DevBuf<double>& da, DevBuf<int64_t>& daoff, DevBuf<int64_t>& doff, DevBuf<double>& dca) {
    CR_REQUIRE(atoms && aoff && ca_rows && offsets, "null argument");
    CR_REQUIRE(p >= 1 && p < (1ll << 31), "number of structures out of range");
    CR_REQUIRE(offsets[0] == 0 && aoff[0] == 0, "offsets must start at 0");
    for (int64_t s = 0; s < p; s++) {
        CR_REQUIRE(offsets[s + 1] >= offsets[s] && aoff[s + 1] >= aoff[s], "offsets must be non-decreasing");
        for (int64_t r = offsets[s]; r < offsets[s + 1]; r++)
            CR_REQUIRE(ca_rows[r] >= 0 && ca_rows[r] < aoff[s + 1] - aoff[s], "a C-alpha row lies outside its structure's atoms");
    }
    CR_REQUIRE(all_finite(atoms, (size_t)aoff[p] * 3), "coordinates contain NaN or infinity");
    DevBuf<int32_t> drow;
    int rc;
    if ((rc = upload(da, atoms, (size_t)aoff[p] * 3, ctx)) || (rc = upload(daoff, aoff, (size_t)p + 1, ctx)) ||
        (rc = upload(doff, offsets, (size_t)p + 1, ctx)) || (rc = upload(drow, ca_rows, (size_t)offsets[p], ctx)))
        return rc;
    CR_HIP(dca.ensure((size_t)offsets[p] * 3 + 3));
    CR_LAUNCH(cr::k_gather_calpha, dim3((unsigned)p), dim3(cr::kWave), 0, ctx->stream, da.p, daoff.p, doff.p, drow.p, dca.p);
    CR_HIP(hipGetLastError());
    // (drow goes back to the block cache only after the device has drained)
    return CR_OK;
}

}  // namespace

extern "C" {

int cr_structure_features(cr_context* ctx, const double* coords, const int64_t* offsets, int64_t num_structures, int64_t width,
                          double* tensors_out, int32_t* idx_out) {
    int rc = set_device(ctx);
    if (rc || (rc = ft_check(coords, offsets, num_structures, width))) return rc;
    CR_REQUIRE(tensors_out && idx_out, "null output");
    const size_t total = (size_t)offsets[num_structures];
    DevBuf<int64_t> doff;
    DevBuf<double> dt;
    DevBuf<int32_t> didx;
    if ((rc = ft_run(ctx, coords, offsets, num_structures, width, doff, &dt, didx))) return rc;
    CR_DOWNLOAD_WAIT(ctx, idx_out, didx.p, sizeof(int32_t) * total);
    CR_DOWNLOAD_WAIT(ctx, tensors_out, dt.p, sizeof(double) * total * (size_t)width);
    return CR_OK;
}

int cr_structure_shapemer_distance_matrix(cr_context* ctx, const double* coords, const int64_t* offsets, int64_t num_structures,
                                          int64_t width, double* tensors_out, int32_t* idx_out, double* out) {
    int rc = set_device(ctx);
    if (rc || (rc = ft_check(coords, offsets, num_structures, width))) return rc;
    CR_REQUIRE(out != nullptr, "null output");
    const size_t total = (size_t)offsets[num_structures];
    const int64_t k = (int64_t)1 << width;
    DevBuf<int64_t> doff;
    DevBuf<double> dt;
    DevBuf<int32_t> didx;
    if ((rc = ft_run(ctx, coords, offsets, num_structures, width, doff, tensors_out ? &dt : nullptr, didx))) return rc;
    // the residue offsets are the CSR offsets of the index lists: straight into the histogram
    ShSide side;
    DevBuf<uint32_t> stat;
    CR_HIP(stat.ensure(2));
    CR_HIP(hipMemsetAsync(stat.p, 0, 2 * sizeof(uint32_t), ctx->stream));
    if ((rc = sh_alloc_counts(side, num_structures, k, ctx))) return rc;
    CR_LAUNCH(cr::k_shapemer_counts, dim3((unsigned)num_structures), dim3(cr::kShThreads), 0, ctx->stream, didx.p, doff.p,
              (int)k, cr::sh_bins_pad(k), side.cnt.p, nullptr, side.n.p, stat.p);
    CR_HIP(hipGetLastError());
    uint32_t st[2];
    if ((rc = sh_stat_fetch(ctx, stat, st)) || (rc = sh_check_stat(st[0]))) return rc;
    if (idx_out) CR_DOWNLOAD_WAIT(ctx, idx_out, didx.p, sizeof(int32_t) * total);
    if (tensors_out) CR_DOWNLOAD_WAIT(ctx, tensors_out, dt.p, sizeof(double) * total * (size_t)width);
    return sh_distances(ctx, side, side, k, st[1], out);
}

int cr_superpose_core_atoms(cr_context* ctx, const double* atoms, const int64_t* atom_offsets, const int32_t* ca_rows,
                            const int64_t* offsets, int64_t P, const int32_t* msa, int64_t W, const int32_t* core,
                            int64_t ncore, int64_t ref, double* atoms_out) {
    int rc = set_device(ctx);
    if (rc) return rc;
    CR_REQUIRE(msa && core && atoms_out, "null argument");
    CR_REQUIRE(P >= 1 && W >= 1 && W <= 65534 && ref >= 0 && ref < P, "bad alignment shape");
    CR_REQUIRE(ncore >= 1 && ncore <= 65534, "superpose_core needs at least one gap-free column");
    DevBuf<double> da, dca, dout, dx1, dcen;
    DevBuf<int64_t> daoff, doff;
    DevBuf<int32_t> dmsa, dcore;
    if ((rc = ft_atoms_upload(ctx, atoms, atom_offsets, ca_rows, offsets, P, da, daoff, doff, dca))) return rc;
    for (int64_t e = 0; e < ncore; e++) {
        CR_REQUIRE(core[e] >= 0 && core[e] < W, "core column outside the alignment");
        for (int64_t s = 0; s < P; s++) {
            const int32_t r = msa[s * W + core[e]];
            CR_REQUIRE(r >= 0 && r < offsets[s + 1] - offsets[s], "a core column holds a gap or an index outside its structure");
        }
    }
    const int64_t natoms = atom_offsets[P];
    if ((rc = upload(dmsa, msa, (size_t)P * W, ctx)) || (rc = upload(dcore, core, (size_t)ncore, ctx))) return rc;
    CR_HIP(dout.ensure((size_t)natoms * 3 + 3));
    CR_HIP(dx1.ensure((size_t)ncore * 3));
    CR_HIP(dcen.ensure(3));
    const size_t lds1 = sizeof(double) * (size_t)cr::kWave * 3;
    CR_LAUNCH(cr::k_core_reference, dim3(1), dim3(cr::kWave), lds1, ctx->stream, dca.p + offsets[ref] * 3, dmsa.p + ref * W,
              dcore.p, (int)ncore, dx1.p, dcen.p);
    CR_HIP(hipGetLastError());
    const size_t lds2 = sizeof(double) * (((size_t)ncore + 3) / 4 * 2 + (size_t)cr::kWave * cr::kMaxAcc);
    if ((rc = allow_lds(cr::k_core_superpose_atoms, lds2))) return rc;
    CR_LAUNCH(cr::k_core_superpose_atoms, dim3((unsigned)P), dim3(cr::kWave), lds2, ctx->stream, dca.p, doff.p, da.p, daoff.p,
              dmsa.p, (int)W, dcore.p, (int)ncore, (int)ref, dx1.p, dcen.p, dout.p);
    CR_HIP(hipGetLastError());
    if (natoms) CR_DOWNLOAD_WAIT(ctx, atoms_out, dout.p, sizeof(double) * (size_t)natoms * 3);
    CR_HIP(hipStreamSynchronize(ctx->stream));
    return CR_OK;
}

int cr_superpose_members_atoms(cr_context* ctx, double* atoms, const int64_t* atom_offsets, const int32_t* ca_rows,
                               const int64_t* offsets, int64_t P, const int32_t* msa, int64_t W, int64_t ref,
                               const int32_t* which, int64_t nwhich) {
    int rc = set_device(ctx);
    if (rc) return rc;
    CR_REQUIRE(msa && (which || nwhich == 0), "null argument");
    CR_REQUIRE(P >= 1 && W >= 1 && W <= 65534 && ref >= 0 && ref < P && nwhich >= 0, "bad alignment shape");
    if (nwhich == 0) return CR_OK;
    for (int64_t b = 0; b < nwhich; b++) CR_REQUIRE(which[b] >= 0 && which[b] < P, "structure index out of range");
    DevBuf<double> da, dca, dout;
    DevBuf<int64_t> daoff, doff;
    DevBuf<int32_t> dmsa, dwhich, dcounts;
    if ((rc = ft_atoms_upload(ctx, atoms, atom_offsets, ca_rows, offsets, P, da, daoff, doff, dca))) return rc;
    for (int64_t s = 0; s < P; s++)
        for (int64_t x = 0; x < W; x++)
            CR_REQUIRE(msa[s * W + x] >= -1 && msa[s * W + x] < offsets[s + 1] - offsets[s], "alignment index outside its structure");
    const int64_t natoms = atom_offsets[P];
    if ((rc = upload(dmsa, msa, (size_t)P * W, ctx)) || (rc = upload(dwhich, which, (size_t)nwhich, ctx))) return rc;
    CR_HIP(dout.ensure((size_t)natoms * 3 + 3));
    CR_HIP(dcounts.ensure((size_t)nwhich));
    if (natoms) CR_HIP(hipMemcpyAsync(dout.p, da.p, sizeof(double) * (size_t)natoms * 3, hipMemcpyDeviceToDevice, ctx->stream));
    const size_t lds = sizeof(double) * (((size_t)W + 3) / 4 * 2 + (size_t)cr::kWave * cr::kMaxAcc);
    if ((rc = allow_lds(cr::k_reference_superpose_atoms, lds))) return rc;
    CR_LAUNCH(cr::k_reference_superpose_atoms, dim3((unsigned)nwhich), dim3(cr::kWave), lds, ctx->stream, dca.p, doff.p, da.p,
              daoff.p, dmsa.p, (int)W, (int)ref, dca.p + offsets[ref] * 3, dwhich.p, dout.p, dcounts.p);
    CR_HIP(hipGetLastError());
    std::vector<int32_t> counts((size_t)nwhich);
    std::vector<double> moved((size_t)natoms * 3);
    CR_DOWNLOAD_WAIT(ctx, counts.data(), dcounts.p, sizeof(int32_t) * (size_t)nwhich);
    if (natoms) CR_DOWNLOAD_WAIT(ctx, moved.data(), dout.p, sizeof(double) * (size_t)natoms * 3);
    for (int64_t b = 0; b < nwhich; b++)
        CR_REQUIRE(counts[(size_t)b] > 3, "a structure shares 3 or fewer alignment columns with the reference (reference: assert len(pos_1) > 3)");
    if (natoms) std::memcpy(atoms, moved.data(), sizeof(double) * (size_t)natoms * 3);
    return CR_OK;
}

}  // extern "C"
