"""``python -m caretta_amd <folder>``: the reference's command line (bin/caretta-cli:14-123) on
``multiple_alignment.align_from_structure_files``.  Flags, defaults and checks are the reference's; the CLI default is
the all-vs-all guide tree (``full = not --fast``)."""
from __future__ import annotations

from pathlib import Path

import typer

app = typer.Typer(add_completion=False)


def input_folder_callback(folder: Path) -> Path:
    if not folder.exists():
        raise typer.BadParameter(f"Folder {folder} does not exist")
    return folder


def output_folder_callback(folder: Path) -> Path:
    if folder.exists():
        raise typer.BadParameter(
            f"Folder {folder} already exists, cowardly refusing to overwrite. Please delete it and try again"
        )
    return folder


def positive_penalty(value: float) -> float:
    if value < 0.0:
        raise typer.BadParameter(f"Value {value} must be positive")
    return value


def features_callback(value: bool) -> bool:
    if value:
        raise typer.BadParameter("aligned DSSP / ProDy feature extraction is not available in caretta_amd")
    return value


@app.command()
def align(
        input_pdb: Path = typer.Argument(..., help="A folder with input protein files", callback=input_folder_callback),
        gap_open_penalty: float = typer.Option(1.0, "-p", help="gap open penalty", callback=positive_penalty),
        gap_extend_penalty: float = typer.Option(0.01, "-e", help="gap extend penalty", callback=positive_penalty),
        consensus_weight: bool = typer.Option(True, "--consensus-weight", "-c",
                                              help="weight well-aligned segments to reduce gaps in these areas"),
        fast: bool = typer.Option(False, "--fast", "-f",
                                  help="Don't use all vs. all pairwise alignment for distance matrix calculation"),
        output: Path = typer.Option(Path("caretta_results"), "--output", "-o", help="folder to store output files",
                                    callback=output_folder_callback),
        fasta: bool = typer.Option(True, help="write alignment in FASTA file format"),
        pdb: bool = typer.Option(True, help="write PDB files superposed according to alignment"),
        threads: int = typer.Option(4, "--threads", "-t", help="number of threads that parse input files (at most 16)"),
        features: bool = typer.Option(False, "--features", callback=features_callback,
                                      help="extract and write aligned features (not available: exits with an error)"),
        only_dssp: bool = typer.Option(False, "--only-dssp", help="extract only DSSP features (unused)"),
        write_class: bool = typer.Option(False, "--class",
                                         help="write MultipleAlignment class with intermediate structures and tree to pickle file"),
        matrix: bool = typer.Option(False, "--matrix",
                                    help="write pre-aligned distance matrix and post-aligned RMSD, coverage and TM-score "
                                         "matrices to files"),
        verbose: bool = typer.Option(True, "--verbose", "-v", help="Control verbosity"),
):
    """
    Align protein structures using Caretta on the GPU.

    Writes the resulting sequence alignment and superposed PDB files to "caretta_results".
    Optionally also outputs the distance matrices, or the python class with intermediate structures made during
    progressive alignment.

    Not the reference's results: per-residue features come from a stand-in descriptor (C-alpha distances to sequence
    neighbours) and a stand-in shapemer rule instead of geometricus, so alignments are outside the parity contract.
    Call align_from_structure_files(features=...) from Python to supply geometricus' features.
    """
    from . import multiple_alignment
    multiple_alignment.align_from_structure_files(
        input_files=input_pdb,
        gap_open_penalty=gap_open_penalty,
        gap_extend_penalty=gap_extend_penalty,
        consensus_weight=consensus_weight,
        full=not fast,
        output_folder=output,
        num_threads=threads,
        write_fasta=fasta,
        write_pdb=pdb,
        write_features=features,
        only_dssp=only_dssp,
        write_class=write_class,
        write_matrix=matrix,
        verbose=verbose,
    )


if __name__ == "__main__":
    app()
