#!/usr/bin/env python3
"""Writes tests/golden/ops_launch_plans.json: the launch plans of ops.py's contraction dispatch (tests/test_ops_plan_cpu.py holds
the recorder and the case table; no GPU, the built library is needed for its host-side `*_supported` shape rules).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ops_plans.py            # rewrite the fixture from ops.py as it is
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_ops_plans.py --time     # host time of the stubbed dispatch, nothing written

The fixture pins behaviour: rewrite it only in a change that is meant to alter a launch plan, never in a refactor.
"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_ops_plan_cpu as T          # noqa: E402


class _ConstLib:
    """Constant answers: 1 from the `*_supported` shape rules, 0 (success) from everything else."""

    def __getattr__(self, name):
        r = 1 if name.endswith('_supported') else 0
        return lambda *a: r


def host_time(calls=4000, repeats=7):
    """Microseconds per call of the stubbed dispatch (no recording, constant library answers, operands built once): the smallest,
    the median and the largest of `repeats` timings of `calls` calls."""
    ops = T.pkg('ops')
    act, S3 = (lambda *s: ops.empty_act(s, 'cpu')), ops.ConvSpec(3, 1, 1, 0)

    def fwd(N, Cc, HW, wino):
        x, out, wp = act(N, Cc, HW, HW), act(N, Cc, HW, HW), T.torch.empty(9 * Cc * Cc)
        kw = {'wino': T._wino_operand(wino, Cc, Cc)} if wino else {}
        return lambda: ops.conv_forward(x, None, wp, Cc, Cc, S3, out=out, **kw)

    def dgrad(N, Cc, HW, wino):
        dy, out, wd = act(N, Cc, HW, HW), act(N, Cc, HW, HW), T.torch.empty(9 * Cc * Cc)
        return lambda: ops.conv_dgrad(dy, wd, Cc, Cc, S3, (HW, HW), out=out, wino=T._wino_operand(wino, Cc, Cc))

    def wgrad(N, Cc, HW):
        dy, x, gw = act(N, Cc, HW, HW), act(N, Cc, HW, HW), T.torch.empty(Cc, Cc, 3, 3)
        return lambda: ops.conv_wgrad(dy, x, None, gw, S3)

    table = {'conv_forward F(2x2,3x3)': fwd(64, 128, 32, '2d'), 'conv_forward F(2x2,3x3) split-K': fwd(256, 256, 4, '2d'),
             'conv_forward F(2,3)': fwd(64, 128, 32, '1d'), 'conv_forward direct folded split-K': fwd(16, 128, 32, None),
             'conv_dgrad F(2x2,3x3)': dgrad(64, 128, 32, '2d'), 'conv_wgrad F(3x3,2x2)': wgrad(64, 128, 32),
             'conv_wgrad F(2,3)': wgrad(32, 128, 64), 'conv_wgrad direct': wgrad(4, 128, 32)}
    out = {}
    with T.recording(ops, [], None, record=False, const_lib=_ConstLib()):
        for name, fn in table.items():
            fn()
            ts = []
            for _ in range(repeats):
                t0 = time.perf_counter()
                for _ in range(calls):
                    fn()
                ts.append((time.perf_counter() - t0) / calls * 1e6)
            out[name] = [round(min(ts), 2), round(sorted(ts)[len(ts) // 2], 2), round(max(ts), 2)]
    return out


if __name__ == '__main__':
    if '--time' in sys.argv:
        print(json.dumps(host_time()))
    else:
        doc = T.record_plans()
        with open(T.FIXTURE, 'w') as f:
            json.dump(doc, f, separators=(',', ':'))
            f.write('\n')
        print('%s: %d cases, %d blocks, %d bytes' % (T.FIXTURE, len(doc['cases']), len(doc['blocks']), os.path.getsize(T.FIXTURE)))
