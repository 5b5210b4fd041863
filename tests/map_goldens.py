"""The reference's `metagraph align --map --count-kmers` goldens on genome.MT.fa, k = 11, reads genome_MT1.fq
(integration_tests/test_align.py:81-87, 115-121, 145-151), shared by tests/test_map_format.py and tests/test_gpu_map_summary.py."""
import os

HERE = os.path.dirname(os.path.abspath(__file__))
K = 11

BASIC_LINES = ["MT-10/1\t1/140/1", "MT-8/1\t140/140/140", "MT-6/1\t140/140/140", "MT-4/1\t0/140/0", "MT-2/1\t140/140/140",
               "MT-11/1\t1/140/1", "MT-11/1\t1/140/1"]
SUBK_LENGTH = 10
SUBK_LINES = ["MT-10/1\t3/141/3", "MT-8/1\t141/141/141", "MT-6/1\t141/141/141", "MT-4/1\t1/141/1", "MT-2/1\t141/141/141",
              "MT-11/1\t4/141/4", "MT-11/1\t3/141/3"]
CANONICAL_LINES = ["MT-10/1\t140/140/140", "MT-8/1\t140/140/140", "MT-6/1\t140/140/140", "MT-4/1\t129/140/129", "MT-2/1\t140/140/139",
                   "MT-11/1\t2/140/2", "MT-11/1\t140/140/140"]


def read_fastq(path=None):
    """(name up to the first white space, like kseq; sequence) of every record"""
    lines = [l.rstrip("\n") for l in open(path or os.path.join(HERE, "golden", "genome_MT1.fq"))]
    return [(lines[i][1:].split()[0], lines[i + 1]) for i in range(0, len(lines) - 3, 4)]


def triples(lines):
    return [tuple(int(x) for x in l.split("\t")[1].split("/")) for l in lines]


def present_full_k(n_discovered, n_kmers, query_len, k, f):
    """DeBruijnGraph::find (sequence_graph.cpp:65-89), restated: Python floats are C doubles, int() truncates like the cast"""
    if query_len < k:
        return False
    return n_kmers - n_discovered <= int(n_kmers * (1 - f))


def present_sub_k(n_discovered, n_kmers, f):
    """cli/align.cpp:139-149, restated"""
    return n_discovered >= int(n_kmers - n_kmers * (1 - f))
