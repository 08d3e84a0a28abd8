"""Alignment blocks of one contig-to-cutout mapping (the reference's kevlar/cigar.py).

A CIGAR is cut into blocks, each with the bases of the target and of the query it covers (None on the side a gap has none), and
the tokenizer's end check then looks at a tail `M (D|I) M`: when the gap and the last match, read as one piece of the sequence
the gap belongs to, start with the other sequence's last block, the alignment could as well have ended in a gap, and the last
block is folded into the third-last one.  The folded block's two sequences are concatenations: one of them skips the gap.

Batches do not come through here: kevlar_amd.varmap reads the end check's answer from the device record (kv_call_scan) and
builds the same blocks by slicing (`AlignmentTokenizer(..., folded=...)`).  Without that answer the check is made here, which
is what single mappings built by hand and the tests use."""
from collections import namedtuple
import re

AlignmentBlock = namedtuple('AlignmentBlock', 'length type target query')

_RUN = re.compile(r'(\d+)([DIM])')


def cigar_blocks(cigar):
    """[(length, type)] of a CIGAR string"""
    return [(int(length), kind) for length, kind in _RUN.findall(cigar)]


class AlignmentTokenizer(object):
    def __init__(self, queryseq, targetseq, cigar, folded=None):
        self._query = queryseq
        self._target = targetseq
        self._origcigar = cigar
        self._cigar = cigar
        self.blocks = self._tokenize()
        self.folded = self._endcheck(folded)

    def _tokenize(self):
        blocks, tpos, qpos = [], 0, 0
        for length, kind in cigar_blocks(self._origcigar):
            target = query = None
            if kind != 'I':
                target = self._target[tpos:tpos + length]
                tpos += length
            if kind != 'D':
                query = self._query[qpos:qpos + length]
                qpos += length
            blocks.append(AlignmentBlock(length, kind, target, query))
        assert tpos == len(self._target) and qpos == len(self._query), 'the CIGAR does not consume both sequences'
        return blocks

    def can_fold(self):
        return len(self.blocks) >= 3 and self.blocks[-1].type == 'M' and self.blocks[-3].type == 'M'

    def _endcheck(self, folded):
        if not self.can_fold():
            return False
        third, gap, last = self.blocks[-3:]
        if folded is None:
            if gap.type == 'D':
                folded = (gap.target + last.target).startswith(last.query)
            else:
                folded = (gap.query + last.query).startswith(last.target)
        if not folded:
            return False
        self.blocks[-3:] = [AlignmentBlock(third.length + last.length, 'M', third.target + last.target, third.query + last.query), gap]
        self._cigar = ''.join('{:d}{:s}'.format(block.length, block.type) for block in self.blocks)
        return True
