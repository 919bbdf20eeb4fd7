"""DSSP features without a GPU: the definitions of DESIGN 4.6 (through the numpy restatement) on ideal geometry built with
synthetic.ideal_backbone, the PDB parser, the C export's declaration and binding, and the refusals of the Python and
command-line surface."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
C1 = ROOT / "tests" / "golden" / "c1_pdb"
sys.path.insert(0, str(Path(__file__).resolve().parent))

import dssp_restatement as R  # noqa: E402

HELIX = (-57.8, -47.0)
STRAND = (-139.0, 135.0)


def _structure(bb, pro=None):
    from caretta_amd.structure_io import DsspAtoms
    bb = np.ascontiguousarray(bb, dtype=np.float64)
    n = len(bb)
    return DsspAtoms(n, np.ones(n, dtype=bool), bb, np.zeros(n, np.int32) if pro is None else np.asarray(pro, np.int32),
                     np.arange(n + 1, dtype=np.int64) * 4, bb.reshape(-1, 3).copy(), np.tile(np.arange(4, dtype=np.int32), n))


def helix(n=20):
    from caretta_amd import synthetic
    return synthetic.ideal_backbone(np.full(n, HELIX[0]), np.full(n, HELIX[1]))


def strands():
    """Two antiparallel ideal strands of 8, the second the first turned 180 degrees about the sheet normal and moved
    4.6 A across and 2 A along: the paired N-O distances are 2.9-3.2 A.  One chain, so there is a break between them."""
    from caretta_amd import synthetic
    n = 8
    a = synthetic.ideal_backbone(np.full(n, STRAND[0]), np.full(n, STRAND[1]))
    ca = a[:, 1]
    c0 = ca.mean(0)
    ax = ca[-1] - ca[0]
    ax /= np.linalg.norm(ax)
    alt = ((a[:, 3] - a[:, 2]) * ((-1.0) ** np.arange(n))[:, None]).mean(0)
    alt -= alt.dot(ax) * ax
    alt /= np.linalg.norm(alt)
    normal = np.cross(ax, alt)
    v = (a - c0).reshape(-1, 3)
    b = (2.0 * np.outer(v @ normal, normal) - v).reshape(n, 4, 3) + c0 + 4.6 * alt - 2.0 * ax
    return np.concatenate([a, b])


def test_helix():
    out = R.dssp_of(_structure(helix()))
    assert list(out["secondary"]) == [""] + ["H"] * 18 + [""]
    assert np.all(out["dssp_NH_O_1_index"][4:] == -4)
    assert np.all(out["dssp_NH_O_1_energy"][4:] < -0.5)
    assert np.all(out["dssp_phi"][1:] == -57.8) and out["dssp_phi"][0] == 360.0
    assert np.all(out["dssp_psi"][:-1] == -47.0) and out["dssp_psi"][-1] == 360.0
    assert out["dssp_kappa"][0] == 360.0 and out["dssp_alpha"][-1] == 360.0 and out["dssp_tco"][0] == 0.0
    assert np.all(out["dssp_tco"][1:] > 0.9)          # helix: consecutive C=O nearly parallel
    # acceptor side: the O of residue i takes the NH of i + 4
    assert np.all(out["dssp_O_NH_1_index"][:16] == 4)


def test_proline_donor_has_no_partner():
    pro = np.zeros(20, np.int32)
    pro[9] = 1
    out = R.dssp_of(_structure(helix(), pro))
    for key in ("dssp_NH_O_1_index", "dssp_NH_O_1_energy", "dssp_NH_O_2_index", "dssp_NH_O_2_energy"):
        assert out[key][9] == 0
    assert out["dssp_NH_O_1_index"][10] == -4
    # residue 5 lost its acceptor partner 9
    assert out["dssp_O_NH_1_index"][5] != 4


def test_break_shifts_the_mapping():
    bb = helix()
    bb[10:] += 100.0                                   # C(9)-N(10) far apart: one break
    full = R.dssp_of(_structure(bb))
    first, second = R.dssp_of(_structure(bb[:10])), R.dssp_of(_structure(bb[10:]))
    for key in R.KEYS:
        assert np.array_equal(full[key][:10], first[key]), key
        assert full[key][10] == 0, key                 # the number the break uses up
        assert np.array_equal(full[key][11:], second[key][:9]), key
    assert full["secondary"][10] == "0"
    assert list(full["secondary"][11:]) == list(second["secondary"][:9])


def _write_pdb(path, bb, names=None, drop=()):
    lines, serial = [], 1
    for i, res in enumerate(bb):
        for a, atom in enumerate(("N", "CA", "C", "O")):
            if (i, atom) in drop:
                continue
            x = res[a]
            resname = names[i] if names else "ALA"
            lines.append(f"ATOM  {serial:5d}  {atom:<3} {resname} A{i + 1:4d}    {x[0]:8.3f}{x[1]:8.3f}{x[2]:8.3f}"
                         f"  1.00  0.00           {atom[0]}")
            serial += 1
        if i == 3:            # a hydrogen, dropped by the parser
            lines.append(f"ATOM  {serial:5d}  H   ALA A{i + 1:4d}    {0.0:8.3f}{0.0:8.3f}{0.0:8.3f}  1.00  0.00           H")
            serial += 1
    Path(path).write_text("\n".join(lines) + "\nEND\n")


def test_incomplete_residue(tmp_path):
    from caretta_amd import structure_io
    bb = np.round(helix(), 3)
    # interior residue 7 without O: it leaves the list, and C(6)-N(8) is a break that uses up its number again
    _write_pdb(tmp_path / "a.pdb", bb, drop={(7, "O")})
    s = structure_io.read_dssp_atoms(tmp_path / "a.pdb")
    assert s.num_residues == 20 and list(np.flatnonzero(~s.complete)) == [7] and len(s.backbone) == 19
    assert len(s.atoms) == 19 * 4 and s.atom_offsets[-1] == 76
    out = R.dssp_of(s)
    assert out["secondary"][7] == "0" and all(out[k][7] == 0 for k in R.KEYS)
    assert out["dssp_phi"][8] == 360.0 and abs(out["dssp_phi"][19] + 57.8) < 0.25
    # residue 0 without O: every value moves one place towards the start, the last position reads 0
    _write_pdb(tmp_path / "b.pdb", bb, drop={(0, "O")})
    s = structure_io.read_dssp_atoms(tmp_path / "b.pdb")
    out = R.dssp_of(s)
    whole = R.dssp_of(_structure(bb[1:]))
    for key in R.KEYS:
        assert np.array_equal(out[key][:19], whole[key]), key
        assert out[key][19] == 0, key
    assert out["secondary"][19] == "0"


def test_far_residue_has_its_own_accessibility():
    bb = helix(12)
    lone = bb[5:6] + np.array([100.0, 0.0, 0.0])
    together = R.dssp_of(_structure(np.concatenate([lone, bb])))     # the lone residue first: position 0
    alone = R.dssp_of(_structure(lone))
    assert together["dssp_acc"][0] == alone["dssp_acc"][0] > 100
    assert np.array_equal(together["dssp_acc"][2:], R.dssp_of(_structure(bb))["dssp_acc"][:11])


def test_antiparallel_strands():
    bb = strands()
    out = R.dssp_of(_structure(bb))
    sec = "".join(c or "-" for c in out["secondary"])
    assert sec == "-EEEEE--0-EEEEE-"
    # the bonded pairs are at hydrogen-bond distance
    d = np.sqrt(((bb[:8, None, 0] - bb[None, 8:, 3]) ** 2).sum(-1))
    assert 2.8 < d.min() < 3.0


def test_sphere_points_match_the_package():
    from caretta_amd import feature_extraction
    p = feature_extraction.sphere_points()
    assert p.shape == (401, 3)
    assert np.array_equal(p, R.sphere_points())
    assert np.allclose(np.linalg.norm(p, axis=1), 1.0)


def test_kringle_parser():
    from caretta_amd import helper, structure_io
    s = structure_io.read_dssp_atoms(C1 / "1kdu.pdb")
    xyz, seq = helper.read_calpha_pdb(C1 / "1kdu.pdb")
    assert s.num_residues == len(xyz) and s.complete.all()
    assert np.array_equal(s.backbone[:, 1], xyz)
    assert len(s.atoms) == s.atom_offsets[-1] and set(np.unique(s.radius_class)) <= {0, 1, 2, 3, 4}
    assert len(s.atoms) == 1319 - 638
    assert s.is_pro.sum() == seq.count("P")


def test_dssp_export_declared_and_bound():
    header = (ROOT / "include" / "caretta_hip.h").read_text()
    declared = set(re.findall(r"\b(cr_[a-z0-9_]+)\s*\(", header))
    from caretta_amd import _capi
    assert "cr_dssp_features" in declared and "cr_dssp_features" in _capi.SIGNATURES
    m = re.search(r"int cr_dssp_features\(([^)]*)\)", header)
    assert len(m.group(1).split(",")) == len(_capi.SIGNATURES["cr_dssp_features"]) == 14
    entry = (ROOT / "__graft_entry__.py").read_text()
    assert '"cr_dssp.h"' in entry


def test_only_dssp_false_raises_first(tmp_path):
    from caretta_amd import feature_extraction
    from caretta_amd.multiple_alignment import get_aligned_features
    missing = tmp_path / "nothing.pdb"
    for call in (lambda: feature_extraction.get_features(missing, tmp_path / "d", only_dssp=False),
                 lambda: feature_extraction.get_features_multiple([missing], tmp_path / "d", only_dssp=False),
                 lambda: get_aligned_features({"nothing": [0]}, tmp_path, tmp_path / "d", 1, only_dssp=False)):
        with pytest.raises(ValueError, match="GNM"):
            call()
    assert list(tmp_path.iterdir()) == []


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "caretta_amd.feature_extraction", *map(str, args)], cwd=str(ROOT),
                          capture_output=True, text=True, timeout=120)


def test_cli_refuses_missing_inputs(tmp_path):
    r = _cli(tmp_path / "missing")
    assert r.returncode != 0 and "not an existing" in r.stderr
    (tmp_path / "res").mkdir()
    r = _cli(tmp_path / "res")
    assert r.returncode != 0 and "result.fasta" in r.stderr
    (tmp_path / "res" / "result.fasta").write_text(">1kdu\nAC-D\n")
    (tmp_path / "res" / "cleaned_pdb").mkdir()
    (tmp_path / "res" / "cleaned_pdb" / "1kdu.pdb").write_text((C1 / "1kdu.pdb").read_text())
    r = _cli(tmp_path / "res")
    assert r.returncode != 0 and "does not match" in r.stderr
    assert not (tmp_path / "res" / "result_features.pkl").exists()


def test_get_features_needs_a_device():
    from caretta_amd import _capi, engine, feature_extraction
    assert engine.device_count() == 0
    with pytest.raises(_capi.CarettaHipError):
        feature_extraction.get_features(C1 / "1kdu.pdb", "unused")
