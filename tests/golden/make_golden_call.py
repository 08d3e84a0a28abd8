#!/usr/bin/env python3
"""Record what the REFERENCE's own `kevlar call` makes of its test data (tests/golden/call/recorded.json).

Runs only in the build container (needs /root/reference, gcc and cythonize); its outputs under tests/golden/call/ are committed
and are what travels to the GPU box.  What it does:

1. copies the reference's small test *data files* for this step into tests/golden/call/ (fixtures: inputs only, no source);
2. imports the reference's call, varmap, cigar and vcf modules from a temporary copy of the package (make_golden.import_reference:
   codec cythonized there, khmer answered by the oracle, pysam and friends stubbed) and answers `kevlar.alignment` with the
   reference's align() compiled into a temporary directory (make_golden_align.compile_reference), wrapped as
   kevlar/alignment.pyx wraps it;
3. for every fixture of tests/call_common.py and every partition records, in the order of the reference's loops, each
   (contig, cutout) pair's score, CIGAR and strand, and the VCF line of every preliminary and every final call (ties of the
   de-duplication pinned to the call made first: see InOrder below); for the forced
   mappings of the reference's test_varmap.py their lines; the VCF header without the date line; str(mapping) of the wasp pair.

Usage:  python tests/golden/make_golden_call.py
"""
import collections
import gzip
import io
import json
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
REFDATA = os.path.join(REF, 'kevlar', 'tests', 'data')
OUT = os.path.join(HERE, 'call')
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import call_common as cc  # noqa: E402
import make_golden  # noqa: E402
import make_golden_align  # noqa: E402


def import_reference(workdir):
    kevlar, scratch = make_golden.import_reference()
    align = make_golden_align.compile_reference(workdir)

    def contig_align(target, query, match=1, mismatch=2, gapopen=5, gapextend=0):
        cigar, score = align(target, query, match, mismatch, gapopen, gapextend)
        return cigar, score

    def align_both_strands(target, query, match=1, mismatch=2, gapopen=5, gapextend=0):      # kevlar/alignment.pyx:27-44
        cigar1, score1 = contig_align(target.sequence, query.sequence, match, mismatch, gapopen, gapextend)
        cigar2, score2 = contig_align(target.sequence, kevlar.revcom(query.sequence), match, mismatch, gapopen, gapextend)
        return (score2, cigar2, -1) if score2 > score1 else (score1, cigar1, 1)

    sys.modules['kevlar.alignment'].contig_align = contig_align
    sys.modules['kevlar.alignment'].align_both_strands = align_both_strands
    kevlar.varmap.align_both_strands = align_both_strands
    return kevlar, scratch


def main():
    shutil.rmtree(OUT, ignore_errors=True)
    for rel in cc.fixture_files():
        dst = os.path.join(OUT, rel)
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        if os.path.exists(os.path.join(REFDATA, rel)):
            shutil.copyfile(os.path.join(REFDATA, rel), dst)
        else:                                                   # a plain-text input stored gzipped
            assert rel.endswith('.gz') and os.path.getsize(os.path.join(REFDATA, rel[:-3])) > cc.GZIPPED, rel
            with open(os.path.join(REFDATA, rel[:-3]), 'rb') as src, gzip.GzipFile(dst, 'wb', mtime=0) as out:
                shutil.copyfileobj(src, out)
    workdir = tempfile.mkdtemp(prefix='kevlar-call-')
    kevlar, scratch = import_reference(workdir)
    kevlar.logstream = io.StringIO()
    seen = []

    class Logged(kevlar.varmap.VariantMapping):
        def __init__(self, contig, cutout, *args, **kwargs):
            super(Logged, self).__init__(contig, cutout, *args, **kwargs)
            if self.nocall:
                seen.append([contig.name, cutout.defline, 0, None, 1])
            else:
                seen.append([contig.name, cutout.defline, self.score, self.tok._origcigar, self.strand])

    kevlar.call.VariantMapping = Logged

    # kevlar/call.py:38-50 keeps the calls of one position in a set of objects hashed by address and takes the first of the
    # longest windows in the set's order: among equally long windows the reference's answer changes from run to run (its own
    # test_cigar_filter_regression accepts either).  The record pins it: the set keeps the order the calls were made in.
    class InOrder(dict):
        def add(self, call):
            self[id(call)] = call

        def __iter__(self):
            return iter(self.values())

    kevlar.call.defaultdict = lambda kind: collections.defaultdict(InOrder if kind is set else kind)
    out = {'fixtures': {}, 'forced': []}
    for fx in cc.FIXTURES:
        parts = []
        for partid, cutouts, contigs in cc.load_partitions(fx, kevlar):
            kwargs = dict(partid=partid, ksize=fx['ksize'], mindist=fx['mindist'], homopolyfilt=fx['homopolyfilt'],
                          maxtargetlen=fx['maxtargetlen'])
            del seen[:]
            prelim = [call.vcf for call in kevlar.call.prelim_call(cutouts, contigs, **kwargs)]
            pairs = list(seen)
            final = [call.vcf for call in kevlar.call.call(cutouts, contigs, **kwargs)]
            final = [prelim.index(line) if line in prelim else line for line in final]      # unchanged calls by index
            parts.append({'partid': partid, 'pairs': pairs, 'prelim': prelim, 'final': final})
        out['fixtures'][fx['name']] = parts
    for contigs, gdnas, score, cigar, ksize in cc.FORCED:
        contig = next(kevlar.parse_augmented_fastx(kevlar.open(cc.data_file(contigs), 'r')))
        cutout = next(kevlar.reference.load_refr_cutouts(kevlar.open(cc.data_file(gdnas), 'r')))
        mapping = kevlar.varmap.VariantMapping(contig, cutout, score, cigar)
        out['forced'].append({'cigar': mapping.cigar, 'vartype': mapping.vartype, 'lines': [call.vcf for call in mapping.call_variants(ksize)]})
    header = io.StringIO()
    kevlar.vcf.VCFWriter(header, source='kevlar::call').write_header()
    out['header'] = [line for line in header.getvalue().split('\n') if line and not line.startswith('##fileDate')]
    contig = next(kevlar.parse_augmented_fastx(kevlar.open(cc.data_file('wasp-pass.contig.augfasta.gz'), 'r')))
    cutout = next(kevlar.reference.load_refr_cutouts(kevlar.open(cc.data_file('wasp.gdna.fa'), 'r')))
    out['wasp_str'] = str(kevlar.varmap.VariantMapping(contig, cutout))
    assert out['wasp_str'] == open(cc.data_file('wasp-align.txt')).read().strip()
    with open(os.path.join(OUT, 'recorded.json'), 'w') as stream:
        # one fixture a line
        stream.write('{"fixtures": {\n' + ',\n'.join('{}: {}'.format(json.dumps(name), json.dumps(out['fixtures'][name], sort_keys=True))
                                                     for name in sorted(out['fixtures'])) + '\n},\n')
        stream.write(',\n'.join('{}: {}'.format(json.dumps(key), json.dumps(out[key], sort_keys=True)) for key in sorted(out) if key != 'fixtures'))
        stream.write('\n}\n')
    shutil.rmtree(workdir, ignore_errors=True)
    shutil.rmtree(scratch, ignore_errors=True)
    npairs = sum(len(part['pairs']) for parts in out['fixtures'].values() for part in parts)
    print('recorded {} alignments of {} fixtures in {}'.format(npairs, len(out['fixtures']), OUT))


if __name__ == '__main__':
    main()
