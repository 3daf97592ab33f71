"""The planted set of the typed cluster CRF's tests and benchmark: three cluster types with 8 domains of their own, 30
background domains, contigs of 150 genes with two 12-gene clusters of one type each (at least 30 genes from each other
and from the ends), and optionally one cluster of two types."""
import numpy as np

TYPES = ["Alpha", "Beta", "Gamma"]
VOCAB = {t: [f"{t}_{k}" for k in range(8)] for t in TYPES}
BACKGROUND = [f"bg_{k}" for k in range(30)]
SPOTS = (35, 95)  # first genes of the two 12-gene clusters of a 150-gene contig: 35 genes from the ends, 48 apart
W, C = 5, 0.15


def contig(rng, name, cluster_types):
    """150 genes; `cluster_types`: the type names of the contig's two clusters.  Returns the genes and the clusters-table
    rows (id, start, end, type)."""
    from gecco_amd import model

    src = model.Source(name)
    genes, rows = [], []
    inside = {}
    for spot, names in zip(SPOTS, cluster_types):
        for i in range(spot, spot + 12):
            inside[i] = names
    for i in range(150):
        names = inside.get(i)
        if names is None:
            doms = [BACKGROUND[int(k)] for k in rng.choice(30, size=int(rng.integers(0, 3)), replace=False)]
        elif len(names) == 1:
            doms = [VOCAB[names[0]][int(k)] for k in rng.choice(8, size=int(rng.integers(1, 3)), replace=False)]
        else:  # a gene of a composite cluster: one domain of each type
            doms = [VOCAB[t][int(rng.integers(0, 8))] for t in names]
        start = 1000 * i + 1
        protein = model.Protein(f"{name}_{i + 1}", None,
                                [model.Domain(d, 10 + 100 * j, 90 + 100 * j, "Pfam", 1e-20, 1e-12) for j, d in enumerate(doms)])
        genes.append(model.Gene(src, start, start + 899, model.Strand.Coding, protein))
    for k, (spot, names) in enumerate(zip(SPOTS, cluster_types)):
        rows.append((f"{name}_bgc{k + 1}", name, genes[spot].start, genes[spot + 11].end, ";".join(sorted(names)), spot))
    return genes, rows


def planted_set(seed, n_contigs, prefix, composite):
    rng = np.random.default_rng(seed)
    genes, rows = [], []
    for c in range(n_contigs):
        kinds = [(TYPES[c % 3],), (TYPES[c % 3],)]
        if composite and c == 0:
            kinds[1] = ("Alpha", "Beta")
        g, r = contig(rng, f"{prefix}{c:02d}", kinds)
        genes += g
        rows += r
    return genes, rows


def cluster_table(rows, types=None):
    from gecco_amd import tables

    return tables.ClusterTable({"sequence_id": [r[1] for r in rows], "cluster_id": [r[0] for r in rows],
                                "start": [r[2] for r in rows], "end": [r[3] for r in rows],
                                "type": [r[4] for r in rows] if types is None else list(types)})
