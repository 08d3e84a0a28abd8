#!/usr/bin/env python3
"""Collect the fixtures of the assembly and alac tests (tests/golden/assemble/) and record what the reference's own tests state
about them (tests/golden/assemble/recorded.json).

Runs only where the reference's checkout is at hand; its outputs under tests/golden/assemble/ are committed.  What it does:

1. copies the reference's small test *data files* for `assemble` and `alac` into tests/golden/assemble/ (inputs only, no source;
   a file that tests/golden/data, localize or call holds already is not copied again: recorded.json says where it is);
2. reads the statements of kevlar/tests/test_assemble.py and kevlar/tests/test_alac.py -- the contigs fermi-lite gave, the
   fixtures that gave none, the positions and alleles of the calls -- out of those two files' literals with `ast`, never by
   running them, and writes them to recorded.json.  Nothing of the reference is compiled or executed.

Usage:  python tests/golden/make_golden_assemble.py
"""
import ast
import glob
import json
import os
import shutil

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
REFDATA = os.path.join(REF, 'kevlar', 'tests', 'data')
OUT = os.path.join(HERE, 'assemble')
MAX_BYTES = 1 << 20

PATTERNS = ['reads2chain.fq.gz', 'fml/*', 'edgeless/*', 'var1.reads.augfastq', 'asmbl-no-edges.augfastq.gz', 'fiveparts*', 'pico-var/*',
            'pico-4.augfastq.gz', 'human-random-pico.fa.gz']
ELSEWHERE = ['data', 'localize', 'call']    # directories of tests/golden that may hold a file already


def parametrize_rows(tree, funcname):
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef) and node.name == funcname:
            for deco in node.decorator_list:
                if isinstance(deco, ast.Call) and getattr(deco.func, 'attr', '') == 'parametrize':
                    return ast.literal_eval(deco.args[0]), ast.literal_eval(deco.args[1])
    raise KeyError(funcname)


def assigned_string(tree, funcname, varname):
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef) and node.name == funcname:
            for stmt in ast.walk(node):
                if isinstance(stmt, ast.Assign) and getattr(stmt.targets[0], 'id', '') == varname:
                    return ast.literal_eval(stmt.value)
    raise KeyError((funcname, varname))


def compared_string(tree, funcname):
    """the literal on the right of `assert contigs[0] == (...)` in funcname"""
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef) and node.name == funcname:
            for stmt in ast.walk(node):
                if isinstance(stmt, ast.Compare) and isinstance(stmt.comparators[0], (ast.Constant, ast.BinOp, ast.JoinedStr)):
                    value = ast.literal_eval(stmt.comparators[0])
                    if isinstance(value, str) and len(value) > 60:
                        return value
    raise KeyError(funcname)


def main():
    shutil.rmtree(OUT, ignore_errors=True)
    os.makedirs(OUT)
    where = {}
    for pattern in PATTERNS:
        for src in sorted(glob.glob(os.path.join(REFDATA, pattern))):
            rel = os.path.relpath(src, REFDATA)
            if os.path.getsize(src) > MAX_BYTES:
                print('left out (too large):', rel)
                continue
            kept = [d for d in ELSEWHERE if os.path.exists(os.path.join(HERE, d, rel))]
            if kept:
                where[rel] = os.path.join(kept[0], rel)
                continue
            dst = os.path.join(OUT, rel)
            os.makedirs(os.path.dirname(dst), exist_ok=True)
            shutil.copyfile(src, dst)
            where[rel] = os.path.join('assemble', rel)
    asm = ast.parse(open(os.path.join(REF, 'kevlar', 'tests', 'test_assemble.py')).read())
    alac = ast.parse(open(os.path.join(REF, 'kevlar', 'tests', 'test_alac.py')).read())
    _, edgeless = parametrize_rows(asm, 'test_assembly_edgeless')
    _, fml = parametrize_rows(asm, 'test_assembly')
    _, pico = parametrize_rows(alac, 'test_pico_calls')
    _, five = parametrize_rows(alac, 'test_alac_single_partition')
    recorded = {
        'files': where,
        'no_contig': ['edgeless/cc{}.afq.gz'.format(cc) for cc in edgeless] + ['asmbl-no-edges.augfastq.gz'],
        'one_contig': dict([('reads2chain.fq.gz', compared_string(asm, 'test_fml_asm')),
                            ('var1.reads.augfastq', assigned_string(asm, 'test_assemble_main', 'contig'))]
                           + [('fml/cc{}.afq.gz'.format(cc), contig) for cc, contig in fml]),
        'fiveparts_partition_4': assigned_string(asm, 'test_assemble_single_part', 'testcontig'),
        # test_alac_single_partition: the call's position is the stated one less 1 (0-based); its PART is the label
        'fiveparts_calls': [{'label': label, 'position': position - 1} for label, position in five],
        # test_pico_calls: ksize=25, delta=50; _pos, _refr, _alt of the one call
        'pico_calls': [{'cc': cc, 'pos': pos, 'ref': ref, 'alt': alt} for cc, pos, ref, alt in pico],
    }
    with open(os.path.join(OUT, 'recorded.json'), 'w') as fh:
        json.dump(recorded, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print('wrote', len(where), 'file locations and recorded.json')


if __name__ == '__main__':
    main()
