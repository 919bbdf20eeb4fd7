// DSSP features (the reference's feature_extraction.get_dssp_features, feature_extraction.py:122-253, which reads them
// from an external mkdssp run through ProDy): backbone H-bond energies, secondary structure, backbone angles and
// Shrake-Rupley accessibility after Kabsch & Sander (1983), every numeric step on the device in FP64.  The definitions,
// and the choices that are ours, are in DESIGN section 4.6; tests/dssp_restatement.py states them again in numpy with
// the same IEEE operations in the same order.  Results are NOT mkdssp's.
//
// Input: a flat batch of structures.  Per complete residue (has N, CA, C and O) the backbone (N, CA, C, O: 12 doubles) and
// a PRO flag; per residue the range of its heavy atoms, per atom its coordinates and radius class; res_off / ca_off
// count complete residues / C-alpha positions per structure.  Included at the end of cr_api.hip.
#pragma once

namespace cr {

constexpr int kDsspThreads = 256;                 // k_dssp_assign, k_dssp_surface (4 waves: 4 atoms)
constexpr int kDsspMaxPoints = 7 * kWave;         // sphere points per atom: 7 per lane at most
constexpr int kDsspCand = 192;                    // occluder candidates per wave held in LDS before a flush
constexpr int kDsspKeys = 14;                     // numeric output rows (DESIGN 4.6 key order)
constexpr double kDsspMaxRadius = 1.87;           // largest atom radius (CA); probe 1.4
constexpr double kDsspProbe = 1.4;
constexpr int64_t kDsspMaxBlocks = 1 << 22;       // workgroups per launch: at most 2^30 work-items at 256 threads

CR_D double dssp_radius(int cls) {
    return cls == 0 ? 1.65 : cls == 1 ? 1.87 : cls == 2 ? 1.76 : cls == 3 ? 1.40 : 1.80;
}

// |a - b| with the squares summed left to right: sqrt((dx*dx + dy*dy) + dz*dz)
CR_D double dssp_d2(const double* a, const double* b) {
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return (dx * dx + dy * dy) + dz * dz;
}
CR_D double dssp_dist(const double* a, const double* b) { return sqrt(dssp_d2(a, b)); }

CR_D double dssp_dot(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
CR_D void dssp_cross(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// dihedral angle p1-p2-p3-p4 in degrees, 360 when undefined (DSSP's formulation)
CR_D double dssp_dihedral(const double* p1, const double* p2, const double* p3, const double* p4) {
    double v12[3], v43[3], z[3], p[3], x[3], y[3];
    for (int a = 0; a < 3; a++) {
        v12[a] = p1[a] - p2[a];
        v43[a] = p4[a] - p3[a];
        z[a] = p2[a] - p3[a];
    }
    dssp_cross(z, v12, p);
    dssp_cross(z, v43, x);
    dssp_cross(z, x, y);
    double u = dssp_dot(x, x), v = dssp_dot(y, y);
    if (u > 0.0 && v > 0.0) {
        u = dssp_dot(p, x) / sqrt(u);
        v = dssp_dot(p, y) / sqrt(v);
        if (u != 0.0 || v != 0.0) return atan2(v, u) * (180.0 / 3.141592653589793);
    }
    return 360.0;
}

// cosine of the angle between p1 - p2 and p3 - p4, 0 when undefined
CR_D double dssp_cosangle(const double* p1, const double* p2, const double* p3, const double* p4) {
    double v12[3], v34[3];
    for (int a = 0; a < 3; a++) {
        v12[a] = p1[a] - p2[a];
        v34[a] = p3[a] - p4[a];
    }
    const double x = dssp_dot(v12, v12) * dssp_dot(v34, v34);
    return x > 0.0 ? dssp_dot(v12, v34) / sqrt(x) : 0.0;
}

// Kabsch-Sander energy of donor NH (N, H) to acceptor CO (C, O); the operand order is the contract
CR_D double dssp_energy(const double* N, const double* H, const double* C, const double* O) {
    const double rON = dssp_dist(O, N), rCH = dssp_dist(C, H), rOH = dssp_dist(O, H), rCN = dssp_dist(C, N);
    if (rON < 0.5 || rCH < 0.5 || rOH < 0.5 || rCN < 0.5) return -9.9;
    const double e = 27.888 * (((1.0 / rON + 1.0 / rCH) - 1.0 / rOH) - 1.0 / rCN);
    return e < -9.9 ? -9.9 : e;
}

// x rounded to 1 / scale (scale 10 or 1000) as format(x, '.1f') / '.3f' and float() give it: the decision against
// the midpoint is exact (the sign of one fma), ties go to even, and n / scale is the correctly rounded decimal.
CR_D double dssp_round_dec(double x, double scale) {
    double k = floor(x * scale);
    if (fma(x, scale, -k) < 0.0) k -= 1.0;                 // now k <= x * scale exactly
    if (fma(x, scale, -(k + 1.0)) >= 0.0) k += 1.0;        // and x * scale < k + 1
    const double d = fma(x, scale, -(k + 0.5));
    double n = d > 0.0 ? k + 1.0 : k;
    if (d == 0.0 && fmod(k, 2.0) != 0.0) n = k + 1.0;
    return n == 0.0 ? copysign(0.0, x) : n / scale;
}

CR_D const double* bb_atom(const double* bb, int64_t r, int a) { return bb + r * 12 + a * 3; }   // a: 0 N, 1 CA, 2 C, 3 O

// One wave per structure: chain breaks (C(i-1)-N(i) > 2.5 A) and DSSP numbers (a ballot scan), then per residue the H
// position, phi / psi / alpha / kappa / tco (raw), the residue's extent around its CA and the atom -> residue map.
__global__ __launch_bounds__(kWave) void k_dssp_backbone(const double* __restrict__ bb, const int64_t* __restrict__ roff,
                                                        const double* __restrict__ atoms,
                                                        const int64_t* __restrict__ raoff,
                                                        int32_t* __restrict__ dnum, double* __restrict__ hpos,
                                                        double* __restrict__ ang, double* __restrict__ ext,
                                                        int32_t* __restrict__ rstruct, int32_t* __restrict__ atom_res,
                                                        int64_t s0) {
    const int s = (int)(s0 + blockIdx.x), lane = threadIdx.x;
    const int64_t b = roff[s];
    const int n = (int)(roff[s + 1] - b);
    int carry = 0;
    for (int base = 0; base < n; base += kWave) {
        const int k = base + lane;
        bool brk = false;
        if (k < n && k > 0) brk = dssp_dist(bb_atom(bb, b + k - 1, 2), bb_atom(bb, b + k, 0)) > 2.5;
        const uint64_t mask = __ballot(brk);
        const int before = __popcll(mask & ((2ull << lane) - 1));        // breaks at or before k in this round
        if (k < n) {
            dnum[b + k] = k + 1 + carry + before;
            rstruct[b + k] = s;
        }
        carry += __popcll(mask);
    }
    __syncthreads();
    // break before residue k <=> its DSSP number jumps by 2
    auto brk_at = [&](int k) { return dnum[b + k] - dnum[b + k - 1] != 1; };
    for (int k = lane; k < n; k += kWave) {
        const int64_t r = b + k;
        const double* N = bb_atom(bb, r, 0);
        const double* CA = bb_atom(bb, r, 1);
        const double* C = bb_atom(bb, r, 2);
        const double* O = bb_atom(bb, r, 3);
        const bool prev = k > 0 && !brk_at(k);
        const bool next = k + 1 < n && !brk_at(k + 1);
        double H[3] = {N[0], N[1], N[2]};
        if (prev) {
            const double* Cp = bb_atom(bb, r - 1, 2);
            const double* Op = bb_atom(bb, r - 1, 3);
            const double v[3] = {Cp[0] - Op[0], Cp[1] - Op[1], Cp[2] - Op[2]};
            const double len = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
            for (int a = 0; a < 3; a++) H[a] = N[a] + v[a] / len;
        }
        for (int a = 0; a < 3; a++) hpos[r * 3 + a] = H[a];
        double phi = 360.0, psi = 360.0, alpha = 360.0, kappa = 360.0, tco = 0.0;
        if (prev) {
            phi = dssp_dihedral(bb_atom(bb, r - 1, 2), N, CA, C);
            tco = dssp_cosangle(C, O, bb_atom(bb, r - 1, 2), bb_atom(bb, r - 1, 3));
        }
        if (next) psi = dssp_dihedral(N, CA, C, bb_atom(bb, r + 1, 0));
        if (prev && next && k + 2 < n && !brk_at(k + 2))
            alpha = dssp_dihedral(bb_atom(bb, r - 1, 1), CA, bb_atom(bb, r + 1, 1), bb_atom(bb, r + 2, 1));
        if (k >= 2 && k + 2 < n && !brk_at(k - 1) && prev && next && !brk_at(k + 2)) {
            // (clamped: rounding can push the cosine of nearly collinear CAs just past +-1)
            const double ck = fmin(1.0, fmax(-1.0, dssp_cosangle(CA, bb_atom(bb, r - 2, 1), bb_atom(bb, r + 2, 1), CA)));
            kappa = atan2(sqrt(1.0 - ck * ck), ck) * (180.0 / 3.141592653589793);
        }
        ang[r * 5 + 0] = phi;
        ang[r * 5 + 1] = psi;
        ang[r * 5 + 2] = alpha;
        ang[r * 5 + 3] = kappa;
        ang[r * 5 + 4] = tco;
        double e2 = 0.0;
        for (int64_t j = raoff[r]; j < raoff[r + 1]; j++) {
            atom_res[j] = (int32_t)r;
            const double d2 = dssp_d2(atoms + j * 3, CA);
            e2 = d2 > e2 ? d2 : e2;
        }
        ext[r] = sqrt(e2);
    }
}

// H-bond energies, every pair of one structure.  One 64-lane workgroup per (structure, tile of 64 own residues); the
// partners' atoms come through LDS a tile at a time.  ACC = false: own residue = donor (NH -> O list), partners =
// acceptors (C, O, CA).  ACC = true: own = acceptor (O -> NH list), partners = donors (N, H, CA, PRO flag).  E is the same
// function of the same operands either way, so both lists agree bit for bit.  Each lane keeps its two lowest negative
// energies in registers (ties: lower partner index first).  hb_idx / hb_e [r * 4 + (ACC ? 2 : 0) + {0, 1}].
template <bool ACC>
__global__ __launch_bounds__(kWave) void k_dssp_hbonds(const double* __restrict__ bb, const double* __restrict__ hpos,
                                                      const int32_t* __restrict__ pro, const int64_t* __restrict__ roff,
                                                      const int64_t* __restrict__ toff, int64_t P,
                                                      int32_t* __restrict__ hb_idx, double* __restrict__ hb_e,
                                                      int64_t blk0) {
    __shared__ double part[9][kWave];            // partner C, O, CA (ACC: N, H, CA), one coordinate plane per row
    __shared__ int32_t part_pro[kWave];
    const int lane = threadIdx.x;
    const int64_t blk = blk0 + blockIdx.x;
    int64_t lo = 0, hi = P;                      // toff[lo] <= blk < toff[lo + 1]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) / 2;
        if (toff[mid] <= blk) lo = mid;
        else hi = mid;
    }
    const int64_t b = roff[lo];
    const int n = (int)(roff[lo + 1] - b);
    const int k = (int)(blk - toff[lo]) * kWave + lane;
    const bool own = k < n;
    double X[9];                                  // own N, H, CA (ACC: C, O, CA)
    bool own_pro = false;
    if (own) {
        const int64_t r = b + k;
        for (int a = 0; a < 3; a++) {
            X[a] = ACC ? bb_atom(bb, r, 2)[a] : bb_atom(bb, r, 0)[a];
            X[3 + a] = ACC ? bb_atom(bb, r, 3)[a] : hpos[r * 3 + a];
            X[6 + a] = bb_atom(bb, r, 1)[a];
        }
        own_pro = pro[r] != 0;
    } else {
        for (int a = 0; a < 9; a++) X[a] = 0.0;
    }
    double e1 = 0.0, e2 = 0.0;
    int i1 = -1, i2 = -1;
    for (int base = 0; base < n; base += kWave) {
        const int m = base + lane;
        __syncthreads();
        if (m < n) {
            const int64_t r = b + m;
            for (int a = 0; a < 3; a++) {
                part[a][lane] = ACC ? bb_atom(bb, r, 0)[a] : bb_atom(bb, r, 2)[a];
                part[3 + a][lane] = ACC ? hpos[r * 3 + a] : bb_atom(bb, r, 3)[a];
                part[6 + a][lane] = bb_atom(bb, r, 1)[a];
            }
            part_pro[lane] = pro[r];
        }
        __syncthreads();
        const int cnt = n - base < kWave ? n - base : kWave;
        if (!own || (!ACC && own_pro)) continue;
        for (int c = 0; c < cnt; c++) {
            const int q = base + c;
            const int d = ACC ? q : k, a = ACC ? k : q;           // donor, acceptor (local indices)
            if (d == a || d == a + 1 || (ACC && part_pro[c])) continue;
            const double pca[3] = {part[6][c], part[7][c], part[8][c]};
            if (dssp_d2(pca, X + 6) >= 81.0) continue;
            const double p0[3] = {part[0][c], part[1][c], part[2][c]};
            const double p1[3] = {part[3][c], part[4][c], part[5][c]};
            const double e = ACC ? dssp_energy(p0, p1, X, X + 3) : dssp_energy(X, X + 3, p0, p1);
            if (!(e < 0.0)) continue;
            if (i1 < 0 || e < e1 || (e == e1 && q < i1)) {
                e2 = e1;
                i2 = i1;
                e1 = e;
                i1 = q;
            } else if (i2 < 0 || e < e2 || (e == e2 && q < i2)) {
                e2 = e;
                i2 = q;
            }
        }
    }
    if (own) {
        const int64_t o = (b + k) * 4 + (ACC ? 2 : 0);
        hb_idx[o] = i1;
        hb_idx[o + 1] = i2;
        hb_e[o] = i1 < 0 ? 0.0 : e1;
        hb_e[o + 1] = i2 < 0 ? 0.0 : e2;
    }
}

// Shrake-Rupley.  One wave per atom (4 per workgroup), lanes over the sphere points (point p = lane + 64 t, t < 7).  The
// wave scans the structure's residues, keeps those whose CA lies within R_i + 3.27 + extent + 0.01 of the atom (only
// they can hold an occluder), and gathers their atoms within R_i + R_j + 0.01 into an LDS list; a full list is tested
// against the points and emptied.  A point is exposed when no other atom j has |x_i + R_i p - x_j|^2 < R_j^2: the
// prefilters only drop atoms that cannot satisfy that, so the result is the brute-force definition's.
__global__ __launch_bounds__(kDsspThreads) void k_dssp_surface(const double* __restrict__ atoms,
                                                              const int32_t* __restrict__ rclass,
                                                              const int64_t* __restrict__ raoff,
                                                              const double* __restrict__ bb, const double* __restrict__ ext,
                                                              const int32_t* __restrict__ rstruct,
                                                              const int32_t* __restrict__ atom_res,
                                                              const int64_t* __restrict__ roff, int64_t natoms,
                                                              const double* __restrict__ points, int npoints, double weight,
                                                              double* __restrict__ area, int64_t a0) {
    __shared__ double cand[kDsspThreads / kWave][4][kDsspCand];   // x, y, z, R_j^2 per candidate
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    const int64_t ai = a0 + (int64_t)blockIdx.x * (kDsspThreads / kWave) + w;
    if (ai >= natoms) return;                                       // wave-uniform
    double (*L)[kDsspCand] = cand[w];
    const int64_t r = atom_res[ai], s = rstruct[r];
    const int64_t rb = roff[s], re = roff[s + 1];
    const double xi[3] = {atoms[ai * 3], atoms[ai * 3 + 1], atoms[ai * 3 + 2]};
    const double Ri = dssp_radius(rclass[ai]) + kDsspProbe;
    double q[7][3];
    uint32_t open = 0;                            // bit t: point lane + 64 t exists and is not occluded yet
#pragma unroll
    for (int t = 0; t < 7; t++) {
        const int p = lane + kWave * t;
        if (p < npoints) {
            open |= 1u << t;
            for (int a = 0; a < 3; a++) q[t][a] = xi[a] + Ri * points[p * 3 + a];
        } else {
            for (int a = 0; a < 3; a++) q[t][a] = 0.0;
        }
    }
    int cnt = 0;
    auto flush = [&]() {
        wave_sync();
        for (int c = 0; c < cnt; c++) {
            if (!__any(open != 0)) break;
            const double xj[3] = {L[0][c], L[1][c], L[2][c]};
            const double rj2 = L[3][c];
#pragma unroll
            for (int t = 0; t < 7; t++)
                if ((open >> t) & 1u)
                    if (dssp_d2(q[t], xj) < rj2) open &= ~(1u << t);
        }
        wave_sync();
        cnt = 0;
    };
    const double reach = Ri + (kDsspMaxRadius + kDsspProbe) + 0.01;
    for (int64_t sb = rb; sb < re; sb += kWave) {
        const int64_t sr = sb + lane;
        bool near = false;
        if (sr < re) {
            const double lim = reach + ext[sr];
            near = dssp_d2(xi, bb_atom(bb, sr, 1)) < lim * lim;
        }
        uint64_t rmask = __ballot(near);
        while (rmask) {
            const int src = __ffsll((unsigned long long)rmask) - 1;
            rmask &= rmask - 1;
            const int64_t S = sb + src;
            for (int64_t jb = raoff[S]; jb < raoff[S + 1]; jb += kWave) {
                const int64_t j = jb + lane;
                bool keep = false;
                double xj[3] = {0.0, 0.0, 0.0}, Rj = 0.0;
                if (j < raoff[S + 1] && j != ai) {
                    for (int a = 0; a < 3; a++) xj[a] = atoms[j * 3 + a];
                    Rj = dssp_radius(rclass[j]) + kDsspProbe;
                    const double lim = Ri + Rj + 0.01;
                    keep = dssp_d2(xi, xj) < lim * lim;
                }
                const uint64_t km = __ballot(keep);
                if (cnt + __popcll(km) > kDsspCand) flush();
                if (keep) {
                    const int slot = cnt + __popcll(km & ((1ull << lane) - 1));
                    L[0][slot] = xj[0];
                    L[1][slot] = xj[1];
                    L[2][slot] = xj[2];
                    L[3][slot] = Rj * Rj;
                }
                cnt += __popcll(km);
            }
        }
    }
    flush();
    int exposed = __popc(open);
    for (int o = 32; o > 0; o >>= 1) exposed += __shfl_xor(exposed, o);
    if (lane == 0) area[ai] = ((Ri * Ri) * weight) * (double)exposed;
}

struct DsspLadder {
    int i0, i1, j0, j1, type, nb;                 // residue ranges of both strands, 1 parallel / 2 antiparallel, bridges
};

// One workgroup per structure: turns, helices, bends, bridges, ladders and bulges, the priority, the decimal rounding,
// and every key written at its C-alpha position (position k <- the complete residue whose DSSP number is k + 1, 0
// otherwise: the reference's mapping, feature_extraction.py:239-252).  The ladders are built by thread 0 in the
// residue order DSSP uses; everything per residue is one thread per residue.
__global__ __launch_bounds__(kDsspThreads) void k_dssp_assign(const int64_t* __restrict__ roff,
                                                             const int64_t* __restrict__ caoff,
                                                             const int64_t* __restrict__ raoff,
                                                             const int32_t* __restrict__ dnum,
                                                             const double* __restrict__ ang,
                                                             const int32_t* __restrict__ hb_idx,
                                                             const double* __restrict__ hb_e,
                                                             const double* __restrict__ area,
                                                             uint8_t* __restrict__ flags, DsspLadder* __restrict__ ladders,
                                                             double* __restrict__ out, int64_t total_ca,
                                                             char* __restrict__ codes, double* __restrict__ raw,
                                                             int64_t s0) {
    const int s = (int)(s0 + blockIdx.x), t = threadIdx.x;
    const int64_t b = roff[s], cb = caoff[s];
    const int n = (int)(roff[s + 1] - b);
    const int64_t L = caoff[s + 1] - cb;
    auto nobreak = [&](int x, int y) { return dnum[b + y] - y == dnum[b + x] - x; };
    // Hbond(a -> d): CO of a to NH of d, d's NH -> O list holds a with E < -0.5
    auto hbond = [&](int a, int d) {
        if (a < 0 || d < 0 || a >= n || d >= n) return false;
        const int64_t o = (b + d) * 4;
        return (hb_idx[o] == a && hb_e[o] < -0.5) || (hb_idx[o + 1] == a && hb_e[o + 1] < -0.5);
    };
    for (int64_t k = t; k < L; k += kDsspThreads) {
        for (int key = 0; key < kDsspKeys; key++) out[key * total_ca + cb + k] = 0.0;
        if (raw)
            for (int key = 0; key < 5; key++) raw[key * total_ca + cb + k] = 0.0;
        codes[cb + k] = '0';
    }
    // flags bits 0..2: n-turn at k (n = 3, 4, 5); bits 4..5: ladder code (1 B, 2 E)
    for (int k = t; k < n; k += kDsspThreads) {
        uint8_t f = 0;
        for (int m = 3; m <= 5; m++)
            if (k + m < n && nobreak(k, k + m) && hbond(k, k + m)) f |= (uint8_t)(1u << (m - 3));
        flags[b + k] = f;
    }
    __syncthreads();
    if (t == 0) {
        DsspLadder* lad = ladders + b * 8;
        int nl = 0;
        auto test_bridge = [&](int i, int j) {
            if (i < 1 || j < 1 || i + 1 >= n || j + 1 >= n || !nobreak(i - 1, i + 1) || !nobreak(j - 1, j + 1)) return 0;
            if ((hbond(i - 1, j) && hbond(j, i + 1)) || (hbond(j - 1, i) && hbond(i, j + 1))) return 1;
            if ((hbond(i, j) && hbond(j, i)) || (hbond(i - 1, j + 1) && hbond(j - 1, i + 1))) return 2;
            return 0;
        };
        for (int i = 1; i + 4 < n; i++) {
            // the only j that can form a bridge with i: Hbond(j -> i), Hbond(j - 1 -> i), Hbond(j -> i + 1),
            // Hbond(j - 1 -> i + 1) -- read from the NH -> O lists of i and i + 1
            int c[8];
            for (int x = 0; x < 2; x++) {
                const int a0 = hb_idx[(b + i) * 4 + x], a1 = hb_idx[(b + i + 1) * 4 + x];
                c[x * 4 + 0] = a0;
                c[x * 4 + 1] = a0 < 0 ? -1 : a0 + 1;
                c[x * 4 + 2] = a1;
                c[x * 4 + 3] = a1 < 0 ? -1 : a1 + 1;
            }
            for (int x = 1; x < 8; x++)                    // ascending j, as DSSP's loop meets them
                for (int y = x; y > 0 && c[y - 1] > c[y]; y--) {
                    const int tmp = c[y];
                    c[y] = c[y - 1];
                    c[y - 1] = tmp;
                }
            for (int x = 0; x < 8; x++) {
                const int j = c[x];
                if (j < i + 3 || j + 1 >= n || (x > 0 && c[x - 1] == j)) continue;
                const int type = test_bridge(i, j);
                if (!type) continue;
                bool found = false;
                for (int l = 0; l < nl && !found; l++) {
                    DsspLadder& g = lad[l];
                    if (g.type != type || i != g.i1 + 1) continue;
                    if (type == 1 && g.j1 + 1 == j) {
                        g.i1 = i;
                        g.j1 = j;
                        g.nb++;
                        found = true;
                    } else if (type == 2 && g.j0 - 1 == j) {
                        g.i1 = i;
                        g.j0 = j;
                        g.nb++;
                        found = true;
                    }
                }
                if (!found) lad[nl++] = DsspLadder{i, i, j, j, type, 1};
            }
        }
        // bulges: DSSP's merge of ladders of one type separated by a gap of <= 1 on one strand and <= 4 on the other
        // (its unsigned differences: `u - v < k` holds only for u >= v)
        auto lt = [](int u, int v, int k) { return u >= v && u - v < k; };
        for (int x = 0; x < nl; x++) {
            if (lad[x].nb == 0) continue;
            for (int y = x + 1; y < nl; y++) {
                DsspLadder& g = lad[x];
                const DsspLadder& h = lad[y];
                if (h.nb == 0) continue;
                const int ibi = g.i0, iei = g.i1, jbi = g.j0, jei = g.j1;
                const int ibj = h.i0, iej = h.i1, jbj = h.j0, jej = h.j1;
                if (g.type != h.type || !nobreak(min(ibi, ibj), max(iei, iej)) || !nobreak(min(jbi, jbj), max(jei, jej)) ||
                    !lt(ibj, iei, 6) || (iei >= ibj && ibi <= iej))
                    continue;
                const bool bulge = g.type == 1 ? ((lt(jbj, jei, 6) && lt(ibj, iei, 3)) || lt(jbj, jei, 3))
                                               : ((lt(jbi, jej, 6) && lt(ibj, iei, 3)) || lt(jbi, jej, 3));
                if (!bulge) continue;
                g.i1 = iej;
                if (g.type == 1) g.j1 = jej;
                else g.j0 = jbj;
                g.nb += h.nb;
                lad[y].nb = 0;
            }
        }
        for (int x = 0; x < nl; x++) {
            const DsspLadder& g = lad[x];
            if (g.nb == 0) continue;
            const uint8_t code = g.nb > 1 ? 2 : 1;
            for (int k = g.i0; k <= g.i1; k++)
                if ((flags[b + k] >> 4) != 2) flags[b + k] = (uint8_t)((flags[b + k] & 15) | (code << 4));
            for (int k = g.j0; k <= g.j1; k++)
                if ((flags[b + k] >> 4) != 2) flags[b + k] = (uint8_t)((flags[b + k] & 15) | (code << 4));
        }
    }
    __syncthreads();
    auto turn = [&](int m, int i) { return i >= 0 && i < n && ((flags[b + i] >> (m - 3)) & 1); };
    for (int k = t; k < n; k += kDsspThreads) {
        const int64_t r = b + k;
        bool helix[3] = {false, false, false}, tt = false;
        for (int m = 3; m <= 5; m++)
            for (int i = k - m + 1; i <= k; i++) {
                if (turn(m, i - 1) && turn(m, i)) helix[m - 3] = true;
                if (i < k && turn(m, i)) tt = true;
            }
        const int lc = flags[r] >> 4;
        const double kappa = ang[r * 5 + 3];
        char code = 0;
        if (helix[1]) code = 'H';
        else if (lc == 2) code = 'E';
        else if (lc == 1) code = 'B';
        else if (helix[0]) code = 'G';
        else if (helix[2]) code = 'I';
        else if (tt) code = 'T';
        else if (kappa != 360.0 && kappa > 70.0) code = 'S';
        const int64_t pos = (int64_t)dnum[r] - 1;
        if (pos >= L) continue;
        const int64_t o = cb + pos;
        codes[o] = code;
        const int32_t* hi = hb_idx + r * 4;       // NH->O 1, NH->O 2, O->NH 1, O->NH 2
        const double* he = hb_e + r * 4;
        const int slot[4] = {0, 4, 2, 6};         // key rows: NH_O_1, NH_O_2, O_NH_1, O_NH_2 (index; energy = + 1)
        for (int x = 0; x < 4; x++) {
            const int p = hi[x];
            out[slot[x] * total_ca + o] = p < 0 ? 0.0 : (double)(dnum[b + p] - dnum[r]);
            out[(slot[x] + 1) * total_ca + o] = p < 0 ? 0.0 : dssp_round_dec(he[x], 10.0);
        }
        double acc = 0.0;
        for (int64_t j = raoff[r]; j < raoff[r + 1]; j++) acc += area[j];
        out[8 * total_ca + o] = floor(acc + 0.5);
        if (raw) {                                // alpha, kappa, phi, psi, tco before rounding
            raw[o] = ang[r * 5 + 2];
            raw[total_ca + o] = kappa;
            raw[2 * total_ca + o] = ang[r * 5 + 0];
            raw[3 * total_ca + o] = ang[r * 5 + 1];
            raw[4 * total_ca + o] = ang[r * 5 + 4];
        }
        out[9 * total_ca + o] = dssp_round_dec(ang[r * 5 + 2], 10.0);      // alpha
        out[10 * total_ca + o] = dssp_round_dec(kappa, 10.0);
        out[11 * total_ca + o] = dssp_round_dec(ang[r * 5 + 0], 10.0);     // phi
        out[12 * total_ca + o] = dssp_round_dec(ang[r * 5 + 1], 10.0);     // psi
        out[13 * total_ca + o] = dssp_round_dec(ang[r * 5 + 4], 1000.0);   // tco
    }
}

}  // namespace cr

extern "C" {

int cr_dssp_features(cr_context* ctx, const double* backbone, const int32_t* is_pro, const int64_t* res_offsets,
                     const int64_t* ca_offsets, const double* atoms, const int32_t* radius_class,
                     const int64_t* atom_offsets, int64_t num_structures, const double* sphere_points, int64_t num_points,
                     double* out, char* secondary_out, double* raw_angles_out) {
    int rc = set_device(ctx);
    if (rc) return rc;
    const int64_t P = num_structures;
    CR_REQUIRE(res_offsets && ca_offsets && atom_offsets && sphere_points && out && secondary_out, "null argument");
    CR_REQUIRE(P >= 1 && P < (1ll << 31), "number of structures out of range");
    CR_REQUIRE(num_points >= 1 && num_points <= cr::kDsspMaxPoints, "number of sphere points must be in [1, 448]");
    CR_REQUIRE(res_offsets[0] == 0 && ca_offsets[0] == 0, "offsets must start at 0");
    for (int64_t s = 0; s < P; s++) {
        CR_REQUIRE(ca_offsets[s + 1] > ca_offsets[s], "a structure without C-alpha positions (ca_offsets must increase)");
        CR_REQUIRE(res_offsets[s + 1] >= res_offsets[s], "res_offsets must be non-decreasing");
        CR_REQUIRE(res_offsets[s + 1] - res_offsets[s] <= ca_offsets[s + 1] - ca_offsets[s],
                   "more complete residues than C-alpha positions in a structure");
    }
    const int64_t R = res_offsets[P], Lt = ca_offsets[P];
    CR_REQUIRE(Lt <= 2147483647ll / 8, "too many residues in one call");
    CR_REQUIRE(R == 0 || (backbone && is_pro), "null backbone");
    CR_REQUIRE(atom_offsets[0] == 0, "atom_offsets must start at 0");
    for (int64_t r = 0; r < R; r++) CR_REQUIRE(atom_offsets[r + 1] >= atom_offsets[r], "atom_offsets must be non-decreasing");
    const int64_t A = atom_offsets[R];
    CR_REQUIRE(A <= 2147483647ll, "at most 2^31 - 1 atoms in one call");
    CR_REQUIRE(A == 0 || (atoms && radius_class), "null atoms");
    for (int64_t j = 0; j < A; j++) CR_REQUIRE(radius_class[j] >= 0 && radius_class[j] <= 4, "radius class outside [0, 4]");
    CR_REQUIRE(R == 0 || all_finite(backbone, (size_t)R * 12), "backbone contains NaN or infinity");
    CR_REQUIRE(A == 0 || all_finite(atoms, (size_t)A * 3), "atoms contain NaN or infinity");
    CR_REQUIRE(all_finite(sphere_points, (size_t)num_points * 3), "sphere points contain NaN or infinity");
    if (R == 0) {
        for (int64_t k = 0; k < Lt; k++) secondary_out[k] = '0';
        std::memset(out, 0, sizeof(double) * (size_t)cr::kDsspKeys * (size_t)Lt);
        if (raw_angles_out) std::memset(raw_angles_out, 0, sizeof(double) * 5 * (size_t)Lt);
        return CR_OK;
    }
    // workgroups of k_dssp_hbonds: a tile of 64 residues of one structure each
    std::vector<int64_t> toff((size_t)P + 1, 0);
    for (int64_t s = 0; s < P; s++) toff[(size_t)s + 1] = toff[(size_t)s] + (res_offsets[s + 1] - res_offsets[s] + cr::kWave - 1) / cr::kWave;
    const int64_t tiles = toff[(size_t)P];
    DevBuf<double> dbb, dat, dpts, dh, dang, dext, dhe, darea, dout, draw;
    DevBuf<int32_t> dpro, dcls, ddn, drs, dares, dhi;
    DevBuf<int64_t> droff, dcaoff, draoff, dtoff;
    DevBuf<uint8_t> dflags;
    DevBuf<cr::DsspLadder> dlad;
    DevBuf<char> dcodes;
    if ((rc = upload(dbb, backbone, (size_t)R * 12, ctx)) || (rc = upload(dpro, is_pro, (size_t)R, ctx)) ||
        (rc = upload(droff, res_offsets, (size_t)P + 1, ctx)) || (rc = upload(dcaoff, ca_offsets, (size_t)P + 1, ctx)) ||
        (rc = upload(draoff, atom_offsets, (size_t)R + 1, ctx)) || (rc = upload(dtoff, toff.data(), (size_t)P + 1, ctx)) ||
        (rc = upload(dpts, sphere_points, (size_t)num_points * 3, ctx)))
        return rc;
    // (no ensure() on an uploaded buffer after its upload: growing a DevBuf hands its block back and takes another)
    if (A && ((rc = upload(dat, atoms, (size_t)A * 3, ctx)) || (rc = upload(dcls, radius_class, (size_t)A, ctx)))) return rc;
    CR_HIP(dares.ensure((size_t)A + 1));
    CR_HIP(darea.ensure((size_t)A + 1));
    CR_HIP(dh.ensure((size_t)R * 3));
    CR_HIP(dang.ensure((size_t)R * 5));
    CR_HIP(dext.ensure((size_t)R));
    CR_HIP(ddn.ensure((size_t)R));
    CR_HIP(drs.ensure((size_t)R));
    CR_HIP(dhi.ensure((size_t)R * 4));
    CR_HIP(dhe.ensure((size_t)R * 4));
    CR_HIP(dflags.ensure((size_t)R));
    CR_HIP(dlad.ensure((size_t)R * 8));
    CR_HIP(dout.ensure((size_t)cr::kDsspKeys * (size_t)Lt));
    CR_HIP(dcodes.ensure((size_t)Lt));
    // Every kernel runs in launches of at most kDsspMaxBlocks workgroups with a base offset: an AQL dispatch holds the
    // grid size in work-items in 32 bits, so one launch over 76 M atoms (4 waves each) would wrap.
    const double weight = (4.0 * M_PI) / (double)num_points;
    const int per = cr::kDsspThreads / cr::kWave;
    const int64_t ablocks = (A + per - 1) / per;
    for (int64_t s0 = 0; s0 < P; s0 += cr::kDsspMaxBlocks) {
        CR_LAUNCH(cr::k_dssp_backbone, dim3((unsigned)std::min<int64_t>(P - s0, cr::kDsspMaxBlocks)), dim3(cr::kWave), 0,
                  ctx->stream, dbb.p, droff.p, dat.p, draoff.p, ddn.p, dh.p, dang.p, dext.p, drs.p, dares.p, s0);
        CR_HIP(hipGetLastError());
    }
    for (int64_t t0 = 0; t0 < tiles; t0 += cr::kDsspMaxBlocks) {
        const unsigned g = (unsigned)std::min<int64_t>(tiles - t0, cr::kDsspMaxBlocks);
        CR_LAUNCH(cr::k_dssp_hbonds<false>, dim3(g), dim3(cr::kWave), 0, ctx->stream, dbb.p, dh.p, dpro.p, droff.p, dtoff.p, P,
                  dhi.p, dhe.p, t0);
        CR_HIP(hipGetLastError());
        CR_LAUNCH(cr::k_dssp_hbonds<true>, dim3(g), dim3(cr::kWave), 0, ctx->stream, dbb.p, dh.p, dpro.p, droff.p, dtoff.p, P,
                  dhi.p, dhe.p, t0);
        CR_HIP(hipGetLastError());
    }
    for (int64_t b0 = 0; b0 < ablocks; b0 += cr::kDsspMaxBlocks) {
        CR_LAUNCH(cr::k_dssp_surface, dim3((unsigned)std::min<int64_t>(ablocks - b0, cr::kDsspMaxBlocks)),
                  dim3(cr::kDsspThreads), 0, ctx->stream, dat.p, dcls.p, draoff.p, dbb.p, dext.p, drs.p, dares.p, droff.p, A,
                  dpts.p, (int)num_points, weight, darea.p, b0 * per);
        CR_HIP(hipGetLastError());
    }
    if (raw_angles_out) CR_HIP(draw.ensure((size_t)5 * (size_t)Lt));
    for (int64_t s0 = 0; s0 < P; s0 += cr::kDsspMaxBlocks) {
        CR_LAUNCH(cr::k_dssp_assign, dim3((unsigned)std::min<int64_t>(P - s0, cr::kDsspMaxBlocks)), dim3(cr::kDsspThreads), 0,
                  ctx->stream, droff.p, dcaoff.p, draoff.p, ddn.p, dang.p, dhi.p, dhe.p, darea.p, dflags.p, dlad.p, dout.p, Lt,
                  dcodes.p, raw_angles_out ? draw.p : nullptr, s0);
        CR_HIP(hipGetLastError());
    }
    CR_DOWNLOAD_WAIT(ctx, out, dout.p, sizeof(double) * (size_t)cr::kDsspKeys * (size_t)Lt);
    CR_DOWNLOAD_WAIT(ctx, secondary_out, dcodes.p, (size_t)Lt);
    if (raw_angles_out) CR_DOWNLOAD_WAIT(ctx, raw_angles_out, draw.p, sizeof(double) * 5 * (size_t)Lt);
    return CR_OK;
}

}  // extern "C"
