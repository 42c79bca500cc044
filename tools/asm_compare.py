#!/usr/bin/env python3
"""Compare the gfx950 device assembly of two builds of one .hip file, kernel by kernel (dev tool; the method of profiles/r07_prune_notes.md section 2).

    hipcc <the build's flags> --cuda-device-only -S old/conv_bfd.hip -o old.s      (same for new.s)
    tools/asm_compare.py old.s new.s [--md] [--diff] [--rename OLD=NEW ...]

--rename pairs a kernel of the old file with one of another name in the new file, both as the table prints them (demangled, without "void " and the
parameter list), e.g.  --rename 'colsum_bf16_kernel=colsum_kernel<unsigned short>'  after a kernel became a template instantiation.

Per kernel: the lines between the kernel's label and its .Lfunc_end, comments and .loc-style directives dropped, .LBBn_m -> .LBB_m, mangled names -> one
token; compared as text.  Registers, spills, scratch and static LDS come from the amdhsa.kernels metadata.  It compares two texts and knows no instruction.
Exit status 1 if a kernel differs or exists on one side only.
"""
import difflib
import re
import shutil
import subprocess
import sys

META = ['vgpr_count', 'sgpr_count', 'vgpr_spill_count', 'sgpr_spill_count', 'private_segment_fixed_size', 'group_segment_fixed_size']


def demangle(names):
    if not names:                                   # (the filter would wait for names on its standard input)
        return {}
    try:
        out = subprocess.run([shutil.which('llvm-cxxfilt') or shutil.which('c++filt') or '/opt/rocm/lib/llvm/bin/llvm-cxxfilt'] + names, capture_output=True, text=True, check=True).stdout.split('\n')
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def kernels(path):
    """{mangled name: (normalised instruction lines, {metadata key: value})}"""
    text = open(path).read()
    meta = {}
    for blk in re.findall(r'- \.agpr_count:.*?\.wavefront_size', text, re.S):
        g = lambda k: (re.search(r'\.%s:\s+(\S+)' % k, blk) or [None, '?'])[1]
        meta[g('name')] = {k: g(k) for k in META}
    lines = text.split('\n')
    out = {}
    for name in meta:
        a = next((i for i, ln in enumerate(lines) if ln.startswith(name + ':')), None)
        if a is None:
            continue
        body = []
        for ln in lines[a + 1:]:
            if ln.startswith('.Lfunc_end'):
                break
            ln = re.sub(r'\s*;.*$', '', ln).strip()
            if not ln or re.match(r'\.(loc|file|cfi_|p2align|section|type|size)\b|\.text$', ln):
                continue
            ln = re.sub(r'\.LBB\d+_(\d+)', r'.LBB_\1', ln)
            ln = re.sub(r'_Z[A-Za-z0-9_]+', 'SYM', ln)
            body.append(ln)
        out[name] = (body, meta[name])
    return out


def by_pretty(ks):
    """The kernels of one file keyed by the name the table prints; overloads that would share it keep their parameter lists."""
    full = demangle(sorted(ks))
    short = {n: re.sub(r'^void |\([^()]*\)$', '', full[n].replace('(anonymous namespace)::', '')) for n in ks}
    twice = {v for v in short.values() if list(short.values()).count(v) > 1}
    return {(full[n] if short[n] in twice else short[n]): ks[n] for n in ks}


def main():
    argv, renames = [], {}
    it = iter(sys.argv[1:])
    for a in it:
        if a == '--rename' or a.startswith('--rename='):
            o, _, n = (next(it, '') if a == '--rename' else a[9:]).partition('=')
            if not o or not n:
                sys.exit(__doc__)
            renames[o] = n
        else:
            argv.append(a)
    args = [a for a in argv if not a.startswith('--')]
    md, show = '--md' in argv, '--diff' in argv
    if len(args) != 2:
        sys.exit(__doc__)
    old, new = by_pretty(kernels(args[0])), by_pretty(kernels(args[1]))
    missing = [o for o in renames if o not in old]
    if missing:
        sys.exit('--rename: not in %s: %s' % (args[0], ', '.join(missing)))
    old = {renames.get(k, k): v for k, v in old.items()}
    was = {v: k for k, v in renames.items()}
    names = sorted(set(old) | set(new))
    bad = 0
    for n in names:
        pretty = n + (' (was %s)' % was[n] if n in was else '')
        if n not in old or n not in new:
            print('%s: only in %s' % (pretty, 'new' if n in new else 'old'))
            bad += 1
            continue
        (bo, mo), (bn, mn) = old[n], new[n]
        same = bo == bn
        bad += not same or mo != mn
        fig = lambda k: mn[k] if mo[k] == mn[k] else '%s -> %s' % (mo[k], mn[k])
        cnt = str(len(bn)) if len(bo) == len(bn) else '%d -> %d' % (len(bo), len(bn))
        cells = [pretty, 'yes' if same else 'NO'] + [fig(k) for k in META] + [cnt]
        print(('| `%s` | ' % cells[0] + ' | '.join(cells[1:]) + ' |') if md else
              '%-64s same %-3s vgpr %-10s sgpr %-10s vspill %-4s sspill %-4s scratch %-4s lds %-4s lines %s' % tuple(cells))
        if show and not same:
            d = list(difflib.unified_diff(bo, bn, 'old', 'new', n=1, lineterm=''))
            print('\n'.join(d[:200]))
            print('... %d diff lines' % len(d))
    print('%d of %d kernels differ' % (bad, len(names)))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
