"""Intervals of the reference genome that a variant contig matches (the reference's kevlar/reference.py:22-32,83-143).

Only the half of that module that needs no aligner exists here: `ReferenceCutout` and `load_refr_cutouts`.  The reference finds
the perfect matches of a contig's seeds with `bwa mem` (kevlar/reference.py:35-80); this project scans the genome on the GPU
instead (kevlar_amd.localize), so there is no index to build and no SAM to parse."""
import re

from kevlar_amd import seqio

_DEFLINE = re.compile(r'(\S+)_(\d+)-(\d+)')


class KevlarInvalidCutoutDeflineError(ValueError):
    pass


class KevlarDeflineSequenceLengthMismatchError(RuntimeError):
    pass


class ReferenceCutout(object):
    """`seqid_start-end`: the span of a cluster of seed matches, widened by delta on both sides, with its sequence.

    The seeds of a contig are its windows of one length; their perfect matches in the genome are sorted by position, split
    where two neighbours lie on different sequences or further apart than X, and each group's span is one cutout."""

    def __init__(self, defline=None, sequence=None):
        self.defline = defline
        self.sequence = sequence
        self._seqid = self._startpos = self._endpos = None
        if defline:
            self.parse_defline(defline)

    def __len__(self):
        return self._endpos - self._startpos

    def parse_defline(self, defline):
        found = _DEFLINE.search(defline)
        if found is None:
            raise KevlarInvalidCutoutDeflineError(defline)
        self._seqid = found.group(1)
        self._startpos, self._endpos = int(found.group(2)), int(found.group(3))
        if self.sequence and len(self.sequence) != len(self):
            raise KevlarDeflineSequenceLengthMismatchError(
                'defline length: {:d}, sequence length: {:d}'.format(len(self), len(self.sequence)))

    @property
    def interval(self):
        return self._seqid, self._startpos, self._endpos

    def local_to_global(self, coordinate):
        return self._startpos + coordinate


def load_refr_cutouts(instream):
    for defline, sequence in seqio.parse_fasta(instream):
        yield ReferenceCutout(defline[1:], sequence)
