"""Sequence ops on the hot path (bionumpy/sequence/__init__.py)."""
from .kmers import get_kmers, count_kmers, KmerEncoder
from .minimizers import get_minimizers, Minimizers
from .dna import get_reverse_complement
from . import translate
from .translate import translate_dna_to_protein
from .string_matcher import match_string
from . import string_matcher
from . import position_weight_matrix
from .position_weight_matrix import PWM, PositionWeightMatrix, get_motif_scores, scan_motifs, MotifScan
from .count_encoded import count_encoded, EncodedCounts, SparseKmerCounts
from . import indexing
from .indexing import KmerIndex, KmerLookup
from . import debruin
from .debruin import DeBruijnGraph, ColoredDeBruijnGraph
from . import bloom_filter
from .bloom_filter import BloomFilter
from . import approximate
from .approximate import find_approximate, trim_adapters, ApproxScan
from . import barcodes
from .barcodes import assign_barcodes, BarcodeAssignment
from . import mates
from .mates import find_mate_overlaps, merge_pairs, MateOverlaps, MergedPairs
from . import alignment
from .alignment import align_pairs, PairwiseAlignments, count_reference_length
from . import seeds
from .seeds import SeedIndex, place_reads, Placements, ReferenceWindows

__all__ = ["get_kmers", "count_kmers", "KmerEncoder", "Minimizers", "PositionWeightMatrix", "get_minimizers", "get_reverse_complement", "translate_dna_to_protein", "translate", "match_string", "string_matcher", "PWM", "get_motif_scores", "scan_motifs", "MotifScan", "position_weight_matrix", "count_encoded", "EncodedCounts", "SparseKmerCounts",
           "KmerIndex", "KmerLookup", "indexing", "debruin", "DeBruijnGraph", "ColoredDeBruijnGraph",
           "bloom_filter", "BloomFilter", "approximate", "find_approximate", "trim_adapters", "ApproxScan",
           "barcodes", "assign_barcodes", "BarcodeAssignment",
           "mates", "find_mate_overlaps", "merge_pairs", "MateOverlaps", "MergedPairs",
           "alignment", "align_pairs", "PairwiseAlignments", "count_reference_length",
           "seeds", "SeedIndex", "place_reads", "Placements", "ReferenceWindows"]
