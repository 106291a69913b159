"""Host side of dp_ups9_fwd (csrc/ups9.hip): the shape rule that restates, argument by argument, what dp_ups9_fwd checks before it launches, and the gate.  The
weight gradient of the nine-product form is not built, so there is no rule or gate of its own to check."""
import itertools

from helpers import pkg


def _ok(N=2, Cin=64, Cout=64, H=8, W=8, **over):
    ops = pkg('ops')
    ldu = (Cout + 3) // 4 * 4
    a = dict(x_img_stride=Cin * H * W, y_img_stride=4 * Cout * H * W, ldu=ldu, u_ptr=0, y_ptr=0, bias_ptr=0)
    a['x_bytes'] = ((N - 1) * a['x_img_stride'] + Cin * H * W) * 4
    a['u_bytes'] = 9 * Cin * ldu * 4
    a.update(over)
    if 'x_img_stride' in over and 'x_bytes' not in over:
        a['x_bytes'] = ((N - 1) * a['x_img_stride'] + Cin * H * W) * 4
    if 'ldu' in over and 'u_bytes' not in over:
        a['u_bytes'] = 9 * Cin * a['ldu'] * 4
    return ops.ups9_fwd_shape_ok(N, Cin, Cout, H, W, a['x_img_stride'], a['y_img_stride'], a['x_bytes'], a['ldu'], a['u_bytes'],
                                 a['u_ptr'], a['y_ptr'], a['bias_ptr'])


def test_shape_rule_case_by_case():
    assert _ok()
    for zero in ('N', 'Cin', 'Cout', 'H', 'W'):
        assert not _ok(**{zero: 0}), zero
    # strides: a channel slice of a wider buffer is fine, overlapping images are not; y needs an even image stride for its 8-byte stores
    assert _ok(x_img_stride=64 * 64 + 37) and not _ok(x_img_stride=64 * 64 - 1)
    assert _ok(y_img_stride=4 * 64 * 64 + 2 * 24) and not _ok(y_img_stride=4 * 64 * 64 - 2)
    assert _ok(N=2, Cin=3, Cout=5, H=1, W=1, y_img_stride=22) and not _ok(N=2, Cin=3, Cout=5, H=1, W=1, y_img_stride=21)      # an odd image stride
    # extents: x must hold its last image, and stay below 2 GiB (bit 31 of a byte offset marks an out-of-image element)
    assert not _ok(x_bytes=((2 - 1) * 64 * 64 + 64 * 64) * 4 - 4)
    assert _ok(x_bytes=(1 << 31) - 4) and not _ok(x_bytes=1 << 31)
    assert not _ok(N=512, Cin=256, Cout=256, H=64, W=64)                               # 2 GiB of x
    # U: exactly [9][Cin][ldu] floats, 16-byte aligned, ldu a multiple of four that covers Cout
    assert _ok(Cout=62) and _ok(Cout=62, ldu=68) and not _ok(Cout=62, ldu=62) and not _ok(Cout=62, ldu=60)
    assert not _ok(u_bytes=9 * 64 * 64 * 4 + 16) and not _ok(u_bytes=9 * 64 * 64 * 4 - 16)
    assert not _ok(u_ptr=8) and _ok(u_ptr=1 << 20)
    assert not _ok(y_ptr=4) and _ok(y_ptr=8) and not _ok(bias_ptr=2) and _ok(bias_ptr=4)
    # channel limits: none of its own beyond U's 2 GiB
    assert _ok(Cin=1, Cout=1) and _ok(Cin=1024, Cout=1024, N=1, H=2, W=2)
    assert not _ok(Cin=8192, Cout=8192, N=1, H=1, W=1)                                 # U of 2.25 GiB
    # pixel numbers are ints below 2^29
    assert not _ok(N=1 << 15, Cin=1, Cout=1, H=128, W=128, x_bytes=(1 << 31) - 4)


def test_gate_wants_nothing_with_the_switch_off(monkeypatch):
    ops = pkg('ops')
    monkeypatch.setattr(ops, 'UPS9', False)
    monkeypatch.setattr(ops, 'UPS9_FWD_GATE_MIN_BLOCKS', 0)
    for N, C, H in itertools.product((1, 4, 128, 256), (64, 128, 180, 256, 512), (4, 8, 16, 64)):
        assert not ops.ups9_fwd_wanted(N, C, C, H, H)
        assert not ops.ups9_dgrad_wanted(N, C, C, H, H)


def test_gate_never_wants_what_the_rule_cannot_take(monkeypatch):
    ops = pkg('ops')
    monkeypatch.setattr(ops, 'UPS9', True)
    wanted = 0
    for floor in (ops.UPS9_FWD_GATE_MIN_BLOCKS, 0):
        monkeypatch.setattr(ops, 'UPS9_FWD_GATE_MIN_BLOCKS', floor)
        for N, Cin, Cout, H, W in itertools.product((0, 1, 3, 128, 256, 4096), (1, 20, 179, 256, 512), (1, 36, 180, 256), (1, 4, 16, 128), (1, 6, 16, 128)):
            if ops.ups9_fwd_wanted(N, Cin, Cout, H, W):
                wanted += 1
                assert _ok(N, Cin, Cout, H, W), (N, Cin, Cout, H, W)
    assert wanted > 0
    monkeypatch.setattr(ops, 'UPS9_FWD_GATE_MIN_BLOCKS', 0)
    assert not ops.ups9_fwd_wanted(512, 256, 256, 64, 64) and not ops.ups9_fwd_wanted(0, 256, 256, 16, 16)
    assert not ops.ups9_fwd_wanted(512, 64, 256, 32, 32)                             # 2 GiB of y
