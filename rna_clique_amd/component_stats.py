"""component_stats: the component census of a written gene matches graph.

    python -m rna_clique_amd.component_stats GRAPH_PKL [--samples N]
        [--statistics [h|m]] [--table OUT.tsv] [--device D]

The statistics of the reference's plot_component_sizes (docs/usage.md), from
graph.pkl alone: the graph's edges go to a graph-only engine, which finds the
components and builds the census on the GPU (census.ComponentTable). The plots
themselves are not drawn here; --table writes the per-component rows they are
made of.
"""
from __future__ import annotations

import argparse
import pickle
import sys

STAT_LABELS = ("Samples", "Total components", "Components >= samples", "Ideal components")


def format_statistics(stats, fmt="h"):
    """The four numbers of ComponentTable.statistics() as text: "h", one
    labelled line each; "m", the numbers on one line, separated by spaces."""
    if fmt == "h":
        return "".join(f"{label}: {value}\n" for label, value in zip(STAT_LABELS, stats))
    if fmt == "m":
        return " ".join(str(v) for v in stats) + "\n"
    raise ValueError("the statistics format is 'h' or 'm'")


def write_table(table, path):
    """ComponentTable.to_frame() as tab-separated values."""
    table.to_frame().to_csv(path, sep="\t", index=False)


def build_parser():
    p = argparse.ArgumentParser(prog="python -m rna_clique_amd.component_stats",
                                description="Census of the connected components of a gene matches graph.")
    p.add_argument("graph", metavar="GRAPH_PKL", help="the pickled gene matches graph (graph.pkl)")
    p.add_argument("--samples", type=int, default=None,
                   help="the number of samples of the analysis (default: the distinct samples among the graph's nodes)")
    p.add_argument("--statistics", nargs="?", const="h", choices=("h", "m"), default=None,
                   help="print samples, total components, components at least as large as the sample count and "
                        "ideal components: h (default) labelled lines, m one line of numbers")
    p.add_argument("--table", default=None, metavar="OUT.tsv", help="write one row per component as TSV")
    p.add_argument("--device", type=int, default=0, help="GPU to use")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    from .similarity import SampleSimilarity
    with open(args.graph, "rb") as f:
        graph = pickle.load(f)
    sim = SampleSimilarity(graph, [], sample_count=args.samples, device=args.device)
    try:
        table = sim.components()
    finally:
        sim.engine.close()
    if args.table:
        write_table(table, args.table)
    if args.statistics:
        sys.stdout.write(format_statistics(table.statistics(), args.statistics))
    return 0


if __name__ == "__main__":
    sys.exit(main())
