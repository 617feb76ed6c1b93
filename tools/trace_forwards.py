#!/usr/bin/env python3
"""Launch-by-launch view of one or two rocprofv3 --kernel-trace CSVs of bench.py: the trace is cut into forwards at the conditioning chain's
first kernel (cond_fc), the steady-state forwards (all but the first `skip` and the last, which the end of the run may cut) are averaged per
launch position: mean, min and standard deviation, wide conv launches in forward order, every kernel's time per forward below.

usage: tools/trace_forwards.py TRACE_DIR [PARENT_TRACE_DIR] [--skip N] [--min-us U]
With two traces the second is the parent: launches are set side by side where both forwards issue the same launch sequence, listed one after
the other where they do not (a merged launch against the launches it replaces)."""
import csv
import glob
import os
import statistics
import sys

WIDE = ('conv_wino', 'conv_tile', 'resblock2_stage', 'conv_post')


def short(n):
    return n.replace('void ', '').replace('(anonymous namespace)::', '').split('(')[0]


def forwards(path, skip):
    """[[(kernel, workgroups, us), ...] per steady-state forward] of the first *_kernel_trace.csv below `path`."""
    f = sorted(glob.glob(os.path.join(path, '**', '*_kernel_trace.csv'), recursive=True))[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r['Start_Timestamp']))
    cuts = [i for i, r in enumerate(rows) if 'cond_fc' in r['Kernel_Name']]
    out = []
    for s, e in zip(cuts[skip:-1], cuts[skip + 1:]):
        out.append([(short(r['Kernel_Name']), int(r['Grid_Size_X']) // max(1, int(r['Workgroup_Size_X'])),
                     (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3) for r in rows[s:e]])
    sig = statistics.mode(tuple((n, w) for n, w, _ in fw) for fw in out)      # (a forward that re-plans or folds differently is left out)
    return [fw for fw in out if tuple((n, w) for n, w, _ in fw) == sig]


def launches(fws, min_us):
    """[(kernel, workgroups, mean, min, sd)] per launch position of the wide kernels, and {kernel: mean us per forward} of all."""
    pos, per = [], {}
    for i, (n, w, _) in enumerate(fws[0]):
        ds = [fw[i][2] for fw in fws]
        per[n] = per.get(n, 0.0) + statistics.fmean(ds)
        if any(k in n for k in WIDE) and statistics.fmean(ds) >= min_us:
            pos.append((n, w, statistics.fmean(ds), min(ds), statistics.pstdev(ds)))
    return pos, per


def main(argv):
    args = [a for a in argv if not a.startswith('--')]
    opt = {argv[i]: argv[i + 1] for i in range(len(argv) - 1) if argv[i].startswith('--')}
    args = [a for a in args if a not in opt.values()]
    skip, min_us = int(opt.get('--skip', 3)), float(opt.get('--min-us', 100))
    views = []
    for label, path in zip(('this commit', 'parent'), args):
        fws = forwards(path, skip)
        pos, per = launches(fws, min_us)
        views.append((label, pos, per))
        print(f'{label}: kernel time per forward {sum(per.values()):.1f} us (mean over {len(fws)} forwards)')
        for n, w, mean, lo, sd in pos:
            print(f'  {mean:8.1f} us (min {lo:7.1f}, sd {sd:5.1f})  {n}  wgs={w}')
    if len(views) == 2:
        (_, a, pa), (_, b, pb) = views
        if [(n, w) for n, w, *_ in a] == [(n, w) for n, w, *_ in b]:
            print('launch by launch (parent -> this commit):')
            for (n, w, m1, l1, s1), (_, _, m0, l0, s0) in zip(a, b):
                print(f'  {n[:40]:40s} wgs={w:6d}  {m0:8.1f} -> {m1:8.1f} us  {100 * (m1 / m0 - 1):+6.2f} %   (min {l0:7.1f} -> {l1:7.1f}; sd {s0:4.1f}, {s1:4.1f})')
        print('every kernel, time per forward (parent -> this commit):')
        for n in sorted(set(pa) | set(pb), key=lambda n: -max(pa.get(n, 0), pb.get(n, 0))):
            m0, m1 = pb.get(n, 0.0), pa.get(n, 0.0)
            pct = f'{100 * (m1 / m0 - 1):+6.2f} %' if m0 and m1 else ''
            print(f'  {n:70s} {m0:8.1f} -> {m1:8.1f} us  {pct}')


if __name__ == '__main__':
    main(sys.argv[1:])
