#!/usr/bin/env python3
"""Writes tests/golden/prune_score_calls.json: per case the count and a chunked running hash of the ordered ops-level calls of pruning
on the CPU stand-ins (tests/test_prune_score_calls_cpu.py holds the recorder, the case table and `summarise`; no GPU).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_prune_score_calls.py              # rewrite the fixture from pruning.py as it is
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_prune_score_calls.py --diff       # the cases that differ from the fixture, nothing written
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_prune_score_calls.py --full FILE  # every record of every case to FILE (not committed)

The fixture pins behaviour: rewrite it only in a change that is meant to alter a call or a score, never in a refactor.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_prune_score_calls_cpu as T          # noqa: E402


def write(doc, path):
    with open(path, 'w') as f:                 # one case per line
        f.write('{\n' + ',\n'.join('%s: %s' % (json.dumps(k), json.dumps(v, separators=(',', ':'))) for k, v in doc.items()) + '\n}\n')
    print('%s: %d cases, %d bytes' % (path, len(doc), os.path.getsize(path)))


if __name__ == '__main__':
    if '--full' in sys.argv:
        write(T.record_all(full=True), sys.argv[sys.argv.index('--full') + 1])
    elif '--diff' in sys.argv:
        with open(T.FIXTURE) as f:
            old = json.load(f)
        new = T.record_all()
        for name in sorted(set(old) | set(new)):
            if old.get(name) != new.get(name):
                print('%s: %s -> %s records' % (name, old.get(name, {}).get('n'), new.get(name, {}).get('n')))
    else:
        write(T.record_all(), T.FIXTURE)
