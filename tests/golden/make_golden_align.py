#!/usr/bin/env python3
"""Record what the REFERENCE's own align() returns for the alignment tests (tests/golden/align/recorded.json).

Runs only in the build container (needs /root/reference and gcc); its outputs under tests/golden/align/ are committed and are
what travels to the GPU box.  What it does:

1. compiles the reference's src/align.c and third-party/ksw2/ksw2_extz.c into a shared object in a temporary directory (never
   into this repository) and calls its align() through ctypes -- the function kevlar/alignment.pyx wraps;
2. copies the reference's small test *data files* for this step into tests/golden/align/ (fixtures: inputs only, no source);
3. records (cigar, score) for every fixture pair on both strands under the four scorings of tests/align_common.py, for the
   literal pair of the reference's test_align, and for the two large seeded pairs of align_common.large_pair (sequences are not
   stored: the generator and the seed are); checks the CIGARs kevlar/tests/test_call.py:77-80 records for pico-2 / pico-7
   against the both-strands winner and stores them.

Usage:  python tests/golden/make_golden_align.py
"""
import ctypes
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
REFDATA = os.path.join(REF, 'kevlar', 'tests', 'data')
OUT = os.path.join(HERE, 'align')
sys.path.insert(0, os.path.dirname(HERE))
import align_common as ac  # noqa: E402

# kevlar/tests/test_call.py:77-80
TEST_CALL_CIGARS = {'pico-7': '10D83M190D75M20I1M', 'pico-2': '10D89M153I75M20I'}


def compile_reference(workdir):
    lib = os.path.join(workdir, 'libkevlaralign.so')
    subprocess.check_call(['gcc', '-O2', '-shared', '-fPIC', '-I', os.path.join(REF, 'inc'), '-I', os.path.join(REF, 'third-party', 'ksw2'),
                           os.path.join(REF, 'src', 'align.c'), os.path.join(REF, 'third-party', 'ksw2', 'ksw2_extz.c'), '-o', lib])
    handle = ctypes.CDLL(lib)
    handle.align.restype = None
    handle.align.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                             ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]

    def align(target, query, match=1, mismatch=2, gapopen=5, gapextend=0):
        cigar = ctypes.create_string_buffer(1 << 18)        # (the reference's wrapper gives it 4096 characters)
        score = ctypes.c_int(0)
        handle.align(target.encode('ascii'), query.encode('ascii'), match, mismatch, gapopen, gapextend, cigar, ctypes.byref(score))
        return cigar.value.decode('ascii'), score.value
    return align


def main():
    shutil.rmtree(OUT, ignore_errors=True)
    for name, tfile, qfile in ac.FIXTURES:
        for rel in (tfile, qfile):
            dst = os.path.join(OUT, rel)
            os.makedirs(os.path.dirname(dst), exist_ok=True)
            shutil.copyfile(os.path.join(REFDATA, rel), dst)
    workdir = tempfile.mkdtemp(prefix='kevlar-align-')
    align = compile_reference(workdir)
    assert align(ac.LITERAL_TARGET, ac.LITERAL_QUERY) == ac.LITERAL_RESULT
    out = {'scorings': [list(s) for s in ac.SCORINGS], 'pairs': {}, 'test_call': {}, 'large': []}
    out['literal'] = {'cigar': ac.LITERAL_RESULT[0], 'score': ac.LITERAL_RESULT[1]}
    for key, target, query in ac.fixture_pairs():
        for scoring in ac.SCORINGS:
            for strand, seq in ((1, query), (-1, ac.rc(query))):
                cigar, score = align(target, seq, *scoring)
                out['pairs'][ac.record_key(key, strand, scoring)] = [cigar, score]
    for name, cigar in TEST_CALL_CIGARS.items():
        winners = []
        for key, target, query in ac.fixture_pairs():
            if key.startswith(name + ':'):
                fwd, rev = align(target, query), align(target, ac.rc(query))
                winners.append(rev[0] if rev[1] > fwd[1] else fwd[0])
        assert cigar in winners, (name, cigar, winners)
        out['test_call'][name] = cigar
    for kind, seed in ac.LARGE:
        target, query = ac.large_pair(kind, seed)
        for strand, seq in ((1, query), (-1, ac.rc(query))):
            cigar, score = align(target, seq)
            out['large'].append({'kind': kind, 'seed': seed, 'tlen': len(target), 'qlen': len(query), 'strand': strand, 'cigar': cigar,
                                 'score': score})
    with open(os.path.join(OUT, 'recorded.json'), 'w') as stream:
        json.dump(out, stream, indent=0, sort_keys=True)
    shutil.rmtree(workdir, ignore_errors=True)
    print('recorded {} fixture alignments and {} large ones in {}'.format(len(out['pairs']), len(out['large']), OUT))


if __name__ == '__main__':
    main()
