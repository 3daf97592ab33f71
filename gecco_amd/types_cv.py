"""Cross-validate the cluster type classifier of a model directory: held-out type predictions for every training cluster.

    python -m gecco_amd.types_cv --model DIR [--splits 10] [--seed 42] [--no-shuffle] [-o types_cv.tsv]

reads ``domains.tsv``, ``types.tsv`` and ``compositions.npz`` of DIR (what ``gecco_amd.train`` writes; GECCO's embedded data
without ``--model``), runs ``types.cross_validate`` (every fold's forest in one launch) and writes one row per cluster, in
input order: ``cluster_id``, ``fold``, ``type``, ``predicted_type`` and one ``{name.lower()}_probability`` column per class
in the order of clusters.tsv.  The per-fold and pooled metrics go to stderr.
"""
import argparse
import sys
from typing import List, Optional, Sequence

from . import types
from .tables import _Table

__all__ = ["TypeCVTable", "cv_table", "main"]


class TypeCVTable(_Table):
    """The table of ``types_cv``: the fixed columns, then the probability columns of its classes; every column is written."""

    COLUMNS = [("cluster_id", str, None), ("fold", int, None), ("type", str, None), ("predicted_type", str, None)]

    def __init__(self, columns=None, classes: Sequence[str] = ()):
        self.COLUMNS = TypeCVTable.COLUMNS + [(col, float, None) for col in types.probability_columns(classes)]
        super().__init__(columns)

    def _dump_columns(self) -> List[str]:
        return [name for name, _, _ in self.COLUMNS]


def cv_table(cluster_ids: Sequence[str], result: "types.TypeCrossValidation") -> TypeCVTable:
    """One row per cluster of `result`, in input order; type strings via ``types.type_string``."""
    names = types.TypeBinarizer(result.classes).inverse_transform(result.truth > 0.5)
    cols = {"cluster_id": list(cluster_ids), "fold": result.fold.tolist(),
            "type": [types.type_string(n) for n in names], "predicted_type": [types.type_string(n) for n in result.predicted]}
    by_column = {f"{name.lower()}_probability": k for k, name in enumerate(result.classes)}
    for col in types.probability_columns(result.classes):
        cols[col] = result.posit[:, by_column[col]]
    return TypeCVTable(cols, classes=result.classes)


def main(argv: Optional[List[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m gecco_amd.types_cv", description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", help="model directory with domains.tsv, types.tsv and compositions.npz (default: GECCO's embedded data)")
    ap.add_argument("--splits", type=int, default=10, help="number of folds (default 10)")
    ap.add_argument("--seed", type=int, default=42, help="seed of the shuffle (default 42)")
    ap.add_argument("--no-shuffle", action="store_true", help="consecutive folds in input order")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("-o", "--output", default="types_cv.tsv")
    args = ap.parse_args(argv)
    path = types.TypeClassifier._embedded_dir() if args.model is None else args.model
    comp, _, ids, labels = types.read_training_data(path)
    classes = sorted(set().union(*labels))
    if len(classes) < 2:
        print(f"{path}: the clusters carry {len(classes)} type(s); the type classifier needs at least two, nothing is fitted",
              file=sys.stderr)
        return 1
    if comp[0][0] != len(labels):
        print(f"{path}: compositions.npz has {comp[0][0]} rows, types.tsv {len(labels)}", file=sys.stderr)
        return 1
    result = types.cross_validate(comp, labels, classes=classes, splits=args.splits, shuffle=not args.no_shuffle, seed=args.seed,
                                  device=args.device)
    cv_table(ids, result).dump(args.output)
    sys.stderr.write(result.summary())
    return 0


if __name__ == "__main__":
    sys.exit(main())
