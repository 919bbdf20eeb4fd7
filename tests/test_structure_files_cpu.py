"""The structure-file entry point without a GPU: the new exports are declared and bound, OutputFiles has the reference's
paths, every input form is parsed and cleaned, the PDB writer touches nothing but the coordinate columns, and the CLI
refuses what the reference refuses before any GPU work."""
import gzip
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
C1 = ROOT / "tests" / "golden" / "c1_pdb"
EXPORTS = {"cr_structure_features", "cr_structure_shapemer_distance_matrix", "cr_superpose_core_atoms",
           "cr_superpose_members_atoms"}


def _cli(*args, cwd):
    env = dict(os.environ, COLUMNS="200", NO_COLOR="1", TERM="dumb", PYTHONPATH=str(ROOT))
    return subprocess.run([sys.executable, "-m", "caretta_amd", *map(str, args)], cwd=cwd, env=env, capture_output=True,
                          text=True, timeout=120)


def test_structure_exports_declared_and_bound():
    header = (ROOT / "include" / "caretta_hip.h").read_text()
    declared = set(re.findall(r"\b(cr_[a-z0-9_]+)\s*\(", header))
    from caretta_amd import _capi
    assert EXPORTS <= declared
    assert EXPORTS <= set(_capi.SIGNATURES)
    for name in EXPORTS:       # one argument per declared parameter
        decl = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", header).group(1)
        assert len(_capi.SIGNATURES[name]) == decl.count(",") + 1, name


def test_output_files_paths():
    from caretta_amd.multiple_alignment import OutputFiles
    out = OutputFiles.from_folder(Path("res"))
    assert out.output_folder == Path("res")
    assert out.fasta_file == Path("res/result.fasta")
    assert out.pdb_folder == Path("res/result_pdb")
    assert out.cleaned_pdb_folder == Path("res/cleaned_pdb")
    assert out.matrix_folder == Path("res/result_matrix")
    assert out.feature_file == Path("res/result_features.pkl")
    assert out.class_file == Path("res/result_class.pkl")
    assert out.tmp_folder == Path("res/tmp")
    assert OutputFiles().output_folder == Path("./caretta_results")


def _atom(serial, name, res, resseq, chain="A", alt=" ", xyz=(1.0, 2.0, 3.0), record="ATOM  "):
    return (f"{record}{serial:5d} {name:<4}{alt}{res:>3} {chain}{resseq:4d}    "
            f"{xyz[0]:8.3f}{xyz[1]:8.3f}{xyz[2]:8.3f}  1.00  0.00           {name[0]}")


def _toy_pdb(path, shift=0.0):
    lines = ["HEADER    TOY"]
    s = 1
    for chain in ("A", "B"):
        for i in range(6):
            x = (3.8 * i + shift, 0.5 * i, 0.0)
            for name, dx in (("N", -1.0), ("CA", 0.0), ("C", 1.0)):
                lines.append(_atom(s, name, "GLY", i + 1, chain, xyz=(x[0] + dx, x[1], x[2])))
                s += 1
        lines.append("TER")
    Path(path).write_text("\n".join(lines) + "\nEND\n")


def test_parse_folder_list_listing_gz_and_chain(tmp_path):
    from caretta_amd import helper, structure_io
    src = tmp_path / "in"
    src.mkdir()
    _toy_pdb(src / "a.pdb")
    _toy_pdb(src / "b.ent", 1.0)
    with gzip.open(src / "c.pdb.gz", "wt") as f:
        f.write((src / "a.pdb").read_text())
    (src / "notes.txt").write_text("not a structure\n")
    # folder
    out = structure_io.parse_protein_files_and_clean(src, tmp_path / "clean1")
    assert [p.name for p in out] == ["a.pdb", "b.pdb", "c.pdb"]
    xyz, seq = helper.read_calpha_pdb(out[0])
    assert seq == "G" * 6 and xyz.shape == (6, 3)
    assert all(line[21] == "A" for line in out[0].read_text().splitlines() if line.startswith("ATOM"))
    # .pdb.gz cleans to the same records as its source
    assert out[2].read_text() == out[0].read_text()
    # list, and (file, chain) tuples
    out = structure_io.parse_protein_files_and_clean([src / "a.pdb", (src / "b.ent", "B")], tmp_path / "clean2", num_threads=4)
    assert [p.name for p in out] == ["a.pdb", "b.pdb"]
    assert all(line[21] == "B" for line in out[1].read_text().splitlines() if line.startswith("ATOM"))
    # a listing file, relative names and ", chain"
    (src / "list.txt").write_text("a.pdb\n\nb.ent, B\n")
    files = structure_io.get_structure_files(src / "list.txt")
    assert [(f.name, c) for f, c in files] == [("a.pdb", None), ("b.ent", "B")]


def test_parse_drops_second_model_and_altloc_b(tmp_path):
    from caretta_amd import structure_io
    lines = ["MODEL        1",
             _atom(1, "N", "ALA", 1), _atom(2, "CA", "ALA", 1, alt="A", xyz=(1, 1, 1)),
             _atom(3, "CA", "ALA", 1, alt="B", xyz=(9, 9, 9)), _atom(4, "CA", "MSE", 2, record="HETATM"),
             _atom(5, "O", "HOH", 3, record="HETATM"), "ENDMDL", "MODEL        2", _atom(6, "CA", "GLY", 1), "ENDMDL", "END"]
    (tmp_path / "m.pdb").write_text("\n".join(lines) + "\n")
    kept = structure_io.clean_pdb_lines(tmp_path / "m.pdb")
    assert [int(line[6:11]) for line in kept] == [1, 2, 4]
    atoms = structure_io.read_pdb_atoms(tmp_path / "m.pdb")
    assert list(atoms.ca_rows) == [1, 3]          # the altloc-A C-alpha and the MSE C-alpha


def test_pdb_id_is_a_value_error_without_network(tmp_path, monkeypatch):
    import socket
    from caretta_amd import structure_io
    from caretta_amd.multiple_alignment import align_from_structure_files

    def no_network(*a, **k):
        raise AssertionError("a network connection was attempted")
    monkeypatch.setattr(socket, "create_connection", no_network)
    monkeypatch.setattr(socket.socket, "connect", no_network)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match="1kdu"):
        structure_io.get_structure_files(["1kdu"])
    with pytest.raises(ValueError, match="4hhb_A"):
        align_from_structure_files("4hhb_A", output_folder=tmp_path / "out", verbose=False)
    assert not (tmp_path / "out").exists()


def test_write_features_raises_before_any_folder(tmp_path):
    from caretta_amd.multiple_alignment import align_from_structure_files
    with pytest.raises(ValueError, match="feature"):
        align_from_structure_files(C1, output_folder=tmp_path / "out", write_features=True, verbose=False)
    assert not (tmp_path / "out").exists()


def test_pdb_writer_changes_only_coordinate_columns(tmp_path):
    from caretta_amd import structure_io
    atoms = structure_io.read_pdb_atoms(C1 / "1kdu.pdb")
    rng = np.random.default_rng(3)
    moved = atoms.coords + rng.uniform(-50, 50, size=atoms.coords.shape)
    structure_io.write_pdb_atoms(tmp_path / "w.pdb", atoms, moved)
    before = (C1 / "1kdu.pdb").read_text().splitlines()
    after = (tmp_path / "w.pdb").read_text().splitlines()
    assert len(before) == len(after)
    for a, b in zip(before, after):
        if a.startswith(("ATOM", "HETATM")):
            assert a[:30] == b[:30] and a[54:] == b[54:]
        else:
            assert a == b
    back = structure_io.read_pdb_atoms(tmp_path / "w.pdb")
    assert np.abs(back.coords - moved).max() <= 5e-4 + 1e-9
    assert np.array_equal(back.ca_rows, atoms.ca_rows)
    with pytest.raises(ValueError, match="does not fit"):
        structure_io.write_pdb_atoms(tmp_path / "x.pdb", atoms, atoms.coords + 1e5)


def test_cli_help_lists_the_reference_flags(tmp_path):
    r = _cli("--help", cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    for flag in ("-p", "-e", "--consensus-weight", "-c", "--fast", "-f", "--output", "-o", "--fasta", "--no-fasta", "--pdb",
                 "--no-pdb", "--threads", "-t", "--features", "--only-dssp", "--class", "--matrix", "--verbose", "-v"):
        assert re.search(r"(^|[\s│,])" + re.escape(flag) + r"(\s|$|,)", r.stdout, re.M), flag
    assert "parity" in r.stdout


def test_cli_refusals(tmp_path):
    (tmp_path / "exists").mkdir()
    r = _cli(C1, "-o", tmp_path / "exists", cwd=tmp_path)
    assert r.returncode != 0 and "cowardly refusing" in r.stdout + r.stderr
    r = _cli(C1, "-p", "-1", "-o", tmp_path / "neg", cwd=tmp_path)
    assert r.returncode != 0 and not (tmp_path / "neg").exists()
    r = _cli(tmp_path / "missing", "-o", tmp_path / "o2", cwd=tmp_path)
    assert r.returncode != 0 and "does not exist" in r.stdout + r.stderr
    r = _cli(C1, "--features", "-o", tmp_path / "o3", cwd=tmp_path)
    assert r.returncode != 0 and not (tmp_path / "o3").exists()


def test_resolved_inputs_parse_again(tmp_path):
    """get_structure_files' own output (file, None) is a valid input: None is the first chain."""
    from caretta_amd import structure_io
    files = structure_io.get_structure_files(C1)
    assert [c for _, c in files] == [None] * 3
    out = structure_io.parse_protein_files_and_clean(files, tmp_path / "clean")
    assert [p.name for p in out] == ["1kdu.pdb", "1pk4.pdb", "1pkr.pdb"]
