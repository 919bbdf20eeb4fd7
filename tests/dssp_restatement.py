"""A plain numpy restatement of the DSSP definitions of DESIGN section 4.6, for the tests only (caretta_amd never imports
it).  It performs the same IEEE operations in the same order as caretta_amd/csrc/cr_dssp.h where results are compared
bit for bit: squared distances ((dx*dx + dy*dy) + dz*dz), the H-bond energy, the per-point occlusion test, the atom
areas and the per-residue sums.  Angles use the same formulas; their last bits may differ (atan2 / acos libraries).

Input: the arrays of structure_io.DsspAtoms (num_residues, backbone (R, 4, 3) of the complete residues, is_pro,
atom_offsets, atoms, radius_class) and, for the mapping onto C-alpha positions, the number of C-alpha residues.
"""
from __future__ import annotations

import math

import numpy as np

KEYS = ("dssp_NH_O_1_index", "dssp_NH_O_1_energy", "dssp_O_NH_1_index", "dssp_O_NH_1_energy",
        "dssp_NH_O_2_index", "dssp_NH_O_2_energy", "dssp_O_NH_2_index", "dssp_O_NH_2_energy",
        "dssp_acc", "dssp_alpha", "dssp_kappa", "dssp_phi", "dssp_psi", "dssp_tco")
ANGLE_KEYS = ("dssp_alpha", "dssp_kappa", "dssp_phi", "dssp_psi", "dssp_tco")
RADII = (1.65, 1.87, 1.76, 1.40, 1.80)
PROBE = 1.4


def sphere_points(n=401):
    golden = (1.0 + math.sqrt(5.0)) / 2.0
    half = (n - 1) // 2
    out = np.empty((n, 3))
    for row, k in enumerate(range(-half, n - half)):
        lat = math.asin(2.0 * k / n)
        lon = math.fmod(k, golden) * 2.0 * math.pi / golden
        out[row] = (math.sin(lon) * math.cos(lat), math.cos(lon) * math.cos(lat), math.sin(lat))
    return out


def d2(a, b):
    """squared distance(s), last axis of length 3: (dx*dx + dy*dy) + dz*dz"""
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def dihedral(p1, p2, p3, p4):
    v12, v43, z = p1 - p2, p4 - p3, p2 - p3
    p, x = cross(z, v12), cross(z, v43)
    y = cross(z, x)
    u, v = dot(x, x), dot(y, y)
    if u > 0.0 and v > 0.0:
        u = dot(p, x) / math.sqrt(u)
        v = dot(p, y) / math.sqrt(v)
        if u != 0.0 or v != 0.0:
            return math.atan2(v, u) * (180.0 / 3.141592653589793)
    return 360.0


def cosangle(p1, p2, p3, p4):
    v12, v34 = p1 - p2, p3 - p4
    x = dot(v12, v12) * dot(v34, v34)
    return dot(v12, v34) / math.sqrt(x) if x > 0.0 else 0.0


def energies(N, H, C, O):
    """E of every donor row (N, H) against every acceptor column (C, O): (R, R)"""
    rON = np.sqrt(d2(O[None, :, :], N[:, None, :]))
    rCH = np.sqrt(d2(C[None, :, :], H[:, None, :]))
    rOH = np.sqrt(d2(O[None, :, :], H[:, None, :]))
    rCN = np.sqrt(d2(C[None, :, :], N[:, None, :]))
    with np.errstate(divide="ignore"):
        e = 27.888 * (((1.0 / rON + 1.0 / rCH) - 1.0 / rOH) - 1.0 / rCN)
    close = (rON < 0.5) | (rCH < 0.5) | (rOH < 0.5) | (rCN < 0.5)
    e = np.where(close, -9.9, e)
    return np.where(e < -9.9, -9.9, e)


def round_dec(x, places):
    return float(format(x, f".{places}f"))


def top_two(e_row, allowed):
    """two lowest negative energies, ties to the lower index: [(index, E)] * 2, (-1, 0.0) for none"""
    cand = [(e_row[q], q) for q in np.flatnonzero(allowed & (e_row < 0.0))]
    cand.sort()
    out = [(q, e) for e, q in cand[:2]]
    return out + [(-1, 0.0)] * (2 - len(out))


def surface_areas(atoms, classes, points):
    """Shrake-Rupley area of every atom by the brute-force definition (every other atom of the structure tested)"""
    R = np.array([RADII[c] for c in classes]) + PROBE
    R2 = R * R
    weight = (4.0 * math.pi) / len(points)
    area = np.zeros(len(atoms))
    for i in range(len(atoms)):
        lim = R[i] + R + 0.01            # atoms farther than this cannot reach a point (the test below decides)
        near = np.flatnonzero(d2(atoms, atoms[i]) < lim * lim)
        near = near[near != i]
        q = atoms[i][None, :] + R[i] * points                          # (NP, 3)
        hit = d2(q[:, None, :], atoms[near][None, :, :]) < R2[near][None, :]
        exposed = int(np.count_nonzero(~hit.any(axis=1)))
        area[i] = ((R[i] * R[i]) * weight) * float(exposed)
    return area


def dssp(num_residues, backbone, is_pro, atom_offsets, atoms, radius_class, points=None):
    """Every key over the C-alpha positions, as cr_dssp_features returns them (secondary: '' no code, '0' no residue)."""
    points = sphere_points() if points is None else points
    bb = np.asarray(backbone, dtype=np.float64).reshape(-1, 4, 3)
    n = len(bb)
    out = {k: np.zeros(num_residues) for k in KEYS}
    out["secondary"] = np.array(["0"] * num_residues, dtype="U1")
    if n == 0:
        return out
    N, CA, C, O = bb[:, 0], bb[:, 1], bb[:, 2], bb[:, 3]
    brk = np.zeros(n, dtype=bool)
    for k in range(1, n):
        brk[k] = math.sqrt(d2(C[k - 1], N[k])) > 2.5
    dnum = np.arange(n) + 1 + np.cumsum(brk)
    H = N.copy()
    for k in range(1, n):
        if not brk[k]:
            v = C[k - 1] - O[k - 1]
            length = math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
            H[k] = N[k] + v / length
    # H-bonds: donor rows, acceptor columns
    E = energies(N, H, C, O)
    ca_ok = d2(CA[None, :, :], CA[:, None, :]) < 81.0
    idx = np.arange(n)
    allowed = ca_ok & (idx[:, None] != idx[None, :]) & (idx[:, None] != idx[None, :] + 1) & (np.asarray(is_pro)[:, None] == 0)
    nho = [top_two(E[d], allowed[d]) for d in range(n)]
    ohn = [top_two(E[:, a], allowed[:, a]) for a in range(n)]

    def nobreak(x, y):
        return dnum[y] - y == dnum[x] - x

    def hbond(a, d):
        if a < 0 or d < 0 or a >= n or d >= n:
            return False
        return any(q == a and e < -0.5 for q, e in nho[d])

    turn = np.zeros((6, n), dtype=bool)
    for m in (3, 4, 5):
        for k in range(n):
            turn[m, k] = k + m < n and nobreak(k, k + m) and hbond(k, k + m)

    def test_bridge(i, j):
        if i < 1 or j < 1 or i + 1 >= n or j + 1 >= n or not nobreak(i - 1, i + 1) or not nobreak(j - 1, j + 1):
            return 0
        if (hbond(i - 1, j) and hbond(j, i + 1)) or (hbond(j - 1, i) and hbond(i, j + 1)):
            return 1
        if (hbond(i, j) and hbond(j, i)) or (hbond(i - 1, j + 1) and hbond(j - 1, i + 1)):
            return 2
        return 0

    ladders = []              # [i0, i1, j0, j1, type, bridges]
    for i in range(1, n - 4):
        for j in range(i + 3, n - 1):
            t = test_bridge(i, j)
            if not t:
                continue
            for g in ladders:
                if g[4] != t or i != g[1] + 1:
                    continue
                if t == 1 and g[3] + 1 == j:
                    g[1], g[3], g[5] = i, j, g[5] + 1
                    break
                if t == 2 and g[2] - 1 == j:
                    g[1], g[2], g[5] = i, j, g[5] + 1
                    break
            else:
                ladders.append([i, i, j, j, t, 1])

    def lt(u, v, k):            # DSSP's unsigned u - v < k
        return u >= v and u - v < k

    for x in range(len(ladders)):
        if ladders[x][5] == 0:
            continue
        for y in range(x + 1, len(ladders)):
            g, h = ladders[x], ladders[y]
            if h[5] == 0:
                continue
            ibi, iei, jbi, jei = g[0], g[1], g[2], g[3]
            ibj, iej, jbj, jej = h[0], h[1], h[2], h[3]
            if (g[4] != h[4] or not nobreak(min(ibi, ibj), max(iei, iej)) or not nobreak(min(jbi, jbj), max(jei, jej))
                    or not lt(ibj, iei, 6) or (iei >= ibj and ibi <= iej)):
                continue
            if g[4] == 1:
                bulge = (lt(jbj, jei, 6) and lt(ibj, iei, 3)) or lt(jbj, jei, 3)
            else:
                bulge = (lt(jbi, jej, 6) and lt(ibj, iei, 3)) or lt(jbi, jej, 3)
            if not bulge:
                continue
            g[1] = iej
            if g[4] == 1:
                g[3] = jej
            else:
                g[2] = jbj
            g[5] += h[5]
            h[5] = 0
    ladder_code = [""] * n
    for g in ladders:
        if g[5] == 0:
            continue
        code = "E" if g[5] > 1 else "B"
        for k in list(range(g[0], g[1] + 1)) + list(range(g[2], g[3] + 1)):
            if ladder_code[k] != "E":
                ladder_code[k] = code

    def turn_at(m, i):
        return 0 <= i < n and turn[m, i]

    area = surface_areas(np.asarray(atoms, dtype=np.float64).reshape(-1, 3), radius_class, points)
    for k in range(n):
        helix = {m: any(turn_at(m, i - 1) and turn_at(m, i) for i in range(k - m + 1, k + 1)) for m in (3, 4, 5)}
        tt = any(turn_at(m, i) for m in (3, 4, 5) for i in range(k - m + 1, k))
        phi = psi = alpha = kappa = 360.0
        tco = 0.0
        prev = k > 0 and not brk[k]
        nxt = k + 1 < n and not brk[k + 1]
        if prev:
            phi = dihedral(C[k - 1], N[k], CA[k], C[k])
            tco = cosangle(C[k], O[k], C[k - 1], O[k - 1])
        if nxt:
            psi = dihedral(N[k], CA[k], C[k], N[k + 1])
        if prev and nxt and k + 2 < n and not brk[k + 2]:
            alpha = dihedral(CA[k - 1], CA[k], CA[k + 1], CA[k + 2])
        if k >= 2 and k + 2 < n and not brk[k - 1] and prev and nxt and not brk[k + 2]:
            ck = min(1.0, max(-1.0, cosangle(CA[k], CA[k - 2], CA[k + 2], CA[k])))
            kappa = math.atan2(math.sqrt(1.0 - ck * ck), ck) * (180.0 / 3.141592653589793)
        if helix[4]:
            code = "H"
        elif ladder_code[k]:
            code = ladder_code[k]
        elif helix[3]:
            code = "G"
        elif helix[5]:
            code = "I"
        elif tt:
            code = "T"
        elif kappa != 360.0 and kappa > 70.0:
            code = "S"
        else:
            code = ""
        pos = dnum[k] - 1
        if pos >= num_residues:
            continue
        out["secondary"][pos] = code
        for name, lists, x in (("NH_O_1", nho, 0), ("NH_O_2", nho, 1), ("O_NH_1", ohn, 0), ("O_NH_2", ohn, 1)):
            q, e = lists[k][x]
            out[f"dssp_{name}_index"][pos] = 0 if q < 0 else dnum[q] - dnum[k]
            out[f"dssp_{name}_energy"][pos] = 0.0 if q < 0 else round_dec(e, 1)
        acc = 0.0
        for j in range(atom_offsets[k], atom_offsets[k + 1]):
            acc += area[j]
        out["dssp_acc"][pos] = math.floor(acc + 0.5)
        out["_raw"] = out.get("_raw", {})
        out["_raw"].setdefault("dssp_alpha", np.full(num_residues, np.nan))[pos] = alpha
        out["_raw"].setdefault("dssp_kappa", np.full(num_residues, np.nan))[pos] = kappa
        out["_raw"].setdefault("dssp_phi", np.full(num_residues, np.nan))[pos] = phi
        out["_raw"].setdefault("dssp_psi", np.full(num_residues, np.nan))[pos] = psi
        out["_raw"].setdefault("dssp_tco", np.full(num_residues, np.nan))[pos] = tco
        out["dssp_alpha"][pos] = round_dec(alpha, 1)
        out["dssp_kappa"][pos] = round_dec(kappa, 1)
        out["dssp_phi"][pos] = round_dec(phi, 1)
        out["dssp_psi"][pos] = round_dec(psi, 1)
        out["dssp_tco"][pos] = round_dec(tco, 3)
    return out


def dssp_of(structure, points=None):
    """dssp() of a structure_io.DsspAtoms"""
    s = structure
    return dssp(s.num_residues, s.backbone, s.is_pro, s.atom_offsets, s.atoms, s.radius_class, points)
