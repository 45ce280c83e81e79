#!/usr/bin/env python3
"""
Is the device code of two source trees the same?  For a refactor that only moves device helpers.

    python tools/compare_device_asm.py TREE_A TREE_B [STEM ...] [--jobs N] [--keep DIR]

Compiles csr_amd/csrc/STEM.hip of each tree (default: every .hip of either tree) to gfx950 assembly with
csr_amd/build.py's flags plus `-S --cuda-device-only`, splits the output by symbol and compares, per kernel,
  - the instruction sequence: comment lines and trailing comments dropped, local labels renumbered in order of
    appearance (a helper that moves between files renumbers every .LBB of the file);
  - the whole .amdhsa_kernel block (registers, LDS, scratch, every enable bit).
Device functions that were not inlined are compared like kernels' instruction sequences.  Data objects are not
compared (the per-file __hip_cuid_* symbol always differs).  The tool only diffs: it looks for no instruction.

Prints one line per file and the names that differ; exits 1 if anything differs or a file is on one side only.
Needs hipcc (HIPCC overrides it) and no GPU.  The trees are paths: check the other commit out with
`git worktree add` or `git archive` first.
"""
import argparse
import concurrent.futures
import glob
import os
import re
import subprocess
import sys
import tempfile

# csr_amd/build.py's compile line
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fvisibility=hidden', '-Wall', '-Wno-unused-function']

LABEL = re.compile(r'\.L[A-Za-z_]+\d+(?:_\d+)?')


def stems_of(tree):
    return {os.path.basename(f)[:-4] for f in glob.glob(os.path.join(tree, 'csr_amd', 'csrc', '*.hip'))}


def compile_asm(tree, stem, out):
    src = os.path.join(tree, 'csr_amd', 'csrc', stem + '.hip')
    cmd = [os.environ.get('HIPCC', 'hipcc')] + FLAGS + ['-S', '--cuda-device-only', src, '-o', out]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if p.returncode != 0:
        sys.stderr.write(p.stdout.decode())
        raise RuntimeError(f'hipcc failed on {src}')
    return out


def split_asm(path):
    """-> ({function symbol: [instruction lines]}, {kernel symbol: [.amdhsa_kernel block lines]})"""
    funcs, blocks = {}, {}
    declared = set()
    name = body = block = None
    labels = {}
    with open(path) as f:
        for raw in f:
            line = raw.split(';', 1)[0].strip()
            if not line:
                continue
            if block is not None:                                   # inside .amdhsa_kernel .. .end_amdhsa_kernel
                if line == '.end_amdhsa_kernel':
                    block = None
                else:
                    block.append(line)
                continue
            m = re.match(r'\.amdhsa_kernel\s+(\S+)', line)
            if m:
                block = blocks.setdefault(m.group(1), [])
                continue
            m = re.match(r'\.type\s+(\S+),@function', line)
            if m:
                declared.add(m.group(1))
                continue
            if body is None:
                if line.endswith(':') and line[:-1] in declared:
                    name, body, labels = line[:-1], [], {}
                continue
            if line.startswith('.Lfunc_end'):
                funcs[name] = body
                name = body = None
                continue
            body.append(LABEL.sub(lambda t: labels.setdefault(t.group(0), f'.L{len(labels)}'), line))
    return funcs, blocks


def compare(a, b):
    """-> (kernels in a, kernels in b, identical kernels, [differing or one-sided symbols, kernel or device function])"""
    fa, ka = split_asm(a)
    fb, kb = split_asm(b)
    same, diff = 0, []
    for s in sorted(set(fa) | set(fb)):
        if s not in fa or s not in fb:
            diff.append(s + ('  (only in B)' if s not in fa else '  (only in A)'))
        elif fa[s] != fb[s]:
            diff.append(s + '  (instructions)')
        elif ka.get(s) != kb.get(s):
            diff.append(s + '  (.amdhsa_kernel block)')
        elif s in ka:
            same += 1
    return len(ka), len(kb), same, diff


def main():
    ap = argparse.ArgumentParser(description=__doc__.strip().split('\n')[0])
    ap.add_argument('tree_a')
    ap.add_argument('tree_b')
    ap.add_argument('stems', nargs='*')
    ap.add_argument('--jobs', type=int, default=16, help='compiles at a time (at most 16)')
    ap.add_argument('--keep', help='leave the .s files in this directory')
    args = ap.parse_args()

    sa, sb = stems_of(args.tree_a), stems_of(args.tree_b)
    stems = sorted(args.stems or (sa | sb))
    bad = 0
    for s in stems:
        if s not in sa or s not in sb:
            print(f'{s}: only in {"B" if s not in sa else "A"}')
            bad += 1
    stems = [s for s in stems if s in sa and s in sb]

    tmp = None
    if args.keep:
        out = args.keep
    else:
        tmp = tempfile.TemporaryDirectory()
        out = tmp.name
    for side in 'ab':
        os.makedirs(os.path.join(out, side), exist_ok=True)
    with concurrent.futures.ThreadPoolExecutor(max(1, min(16, args.jobs))) as ex:
        jobs = {(s, side): ex.submit(compile_asm, tree, s, os.path.join(out, side, s + '.s'))
                for s in stems for side, tree in (('a', args.tree_a), ('b', args.tree_b))}
        paths = {key: j.result() for key, j in jobs.items()}

    tot = [0, 0, 0, 0]
    for s in stems:
        na, nb, same, diff = compare(paths[(s, 'a')], paths[(s, 'b')])
        print(f'{s}: kernels {na} / {nb}, identical {same}, different {len(diff)}')
        for d in diff:
            print(f'    {d}')
        bad += len(diff) + (na != nb)
        for i, v in enumerate((na, nb, same, len(diff))):
            tot[i] += v
    print(f'total: kernels {tot[0]} / {tot[1]}, identical {tot[2]}, different {tot[3]}')
    if tmp:
        tmp.cleanup()
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
