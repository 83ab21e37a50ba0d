"""Deterministic mode, the part that needs no GPU: the process-wide switch (C and Python), the environment switch, the refusals of the
entry points that have no scratch, and the size functions.

With the mode on every float sum of the training path that more than one block adds to has a fixed order (include/titok_hip.h,
ttv_set_deterministic).  The four public ops without a workspace argument get a sibling *_det with (scratch, scratch_bytes); the
plain entry point then returns TTV_ERR_INVALID before it looks at anything else, so these calls pass null pointers and never reach
the GPU.  The tower backward takes its block partials from the workspace, whose size function grows while the mode is on and
returns exactly today's value while it is off.
"""
import ctypes as C
import os
import subprocess
import sys

import pytest

import titok_video_amd
from titok_video_amd import _lib

from tests.test_recompute_cpu import BATCHES, batch_for, dims_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def handle():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _lib.lib()


@pytest.fixture()
def mode(handle):
    """Hands the library over with the mode off and puts back what it found."""
    before = handle.ttv_set_deterministic(0)
    yield handle
    handle.ttv_set_deterministic(before)


def test_set_returns_the_previous_value_and_get_reads_it(mode):
    h = mode
    assert h.ttv_get_deterministic() == 0
    assert h.ttv_set_deterministic(1) == 0
    assert h.ttv_get_deterministic() == 1
    assert h.ttv_set_deterministic(7) == 1          # any non-zero value is "on"
    assert h.ttv_get_deterministic() == 1
    assert h.ttv_set_deterministic(0) == 1
    assert h.ttv_get_deterministic() == 0
    assert h.ttv_set_deterministic(0) == 0


def test_python_functions_reach_the_library(mode):
    h = mode
    assert titok_video_amd.is_deterministic() is False
    assert titok_video_amd.set_deterministic(True) is False
    assert h.ttv_get_deterministic() == 1 and titok_video_amd.is_deterministic() is True
    assert titok_video_amd.set_deterministic(False) is True
    assert h.ttv_get_deterministic() == 0


@pytest.mark.parametrize("value,expect", [(None, 0), ("0", 0), ("1", 1)])
def test_environment_switch_is_applied_when_the_library_is_loaded(handle, value, expect):
    env = {k: v for k, v in os.environ.items() if k != "TTV_DETERMINISTIC"}
    if value is not None:
        env["TTV_DETERMINISTIC"] = value
    out = subprocess.run([sys.executable, "-c", "from titok_video_amd import _lib; print(_lib.lib().ttv_get_deterministic())"],
                         cwd=ROOT, env=env, capture_output=True, text=True, check=True)
    assert int(out.stdout.strip()) == expect


PLAIN = {
    # entry point -> (arguments that touch nothing, the sibling its message must name)
    "ttv_l1_loss": ((None, None, None, None, 0, 0, None, None), b"ttv_l1_loss_det"),
    "ttv_sq_err_accumulate": ((None, None, None, 0, 0, 1, None, None), b"ttv_sq_err_accumulate_det"),
    "ttv_vq_lookup_backward": ((None, 0, 5, None, 0, 5, None, 5, None), b"ttv_vq_lookup_backward_det"),
    "ttv_rmsnorm_backward": ((None, 256, None, 256, None, None, 256, None, 0, 256, 1e-5, 0, None), b"ttv_rmsnorm_backward_det"),
    "ttv_rmsnorm_backward_chain": ((None, 256, None, 256, None, None, None, 256, None, 256, None, None, 1.0, None, 256, 0, 256, 1e-5, 0,
                                    None), b"ttv_rmsnorm_backward_chain_det"),
}


@pytest.mark.parametrize("name", sorted(PLAIN))
def test_scratchless_entry_points_refuse_under_the_mode_and_name_their_sibling(mode, name):
    h = mode
    args, sibling = PLAIN[name]
    assert getattr(h, name)(*args) == 0              # mode off, zero rows / clips: accepted, nothing to launch
    h.ttv_set_deterministic(1)
    assert getattr(h, name)(*args) == 1              # TTV_ERR_INVALID
    msg = h.ttv_error_string()
    assert sibling in msg and b"deterministic" in msg, msg
    assert sibling.decode() in _lib.SYMBOLS


def test_siblings_check_their_scratch_before_any_launch(mode):
    """Mode on, a gain gradient wanted, no scratch: refused with the number of bytes it needs (no pointer is followed)."""
    h = mode
    h.ttv_set_deterministic(1)
    need = h.ttv_rmsnorm_backward_det_scratch_bytes(300, 256)
    fake = C.c_void_p(256)          # non-null, never dereferenced
    rc = h.ttv_rmsnorm_backward_det(fake, 256, fake, 256, fake, fake, 256, fake, 300, 256, 1e-5, 0, None, None, None, None, 0, None)
    assert rc == 1 and str(need).encode() in h.ttv_error_string()
    rc = h.ttv_rmsnorm_backward_det(fake, 256, fake, 256, fake, fake, 256, fake, 300, 256, 1e-5, 0, None, None, None, fake, need - 1, None)
    assert rc == 1 and b"scratch" in h.ttv_error_string()


@pytest.mark.parametrize("size", sorted(BATCHES))
@pytest.mark.parametrize("dtype", [_lib.TTV_BF16, _lib.TTV_F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("kind", [_lib.TTV_ENCODER, _lib.TTV_DECODER], ids=["encoder", "decoder"])
def test_tower_workspace_grows_only_while_the_mode_is_on(mode, kind, dtype, size):
    h = mode
    d, b = dims_for(size, kind, dtype), batch_for(size)

    def sizes():
        return (h.ttv_tower_bwd_workspace_bytes(C.byref(d), C.byref(b)),
                h.ttv_tower_bwd_workspace_bytes_ex(C.byref(d), C.byref(b), _lib.TTV_TAPE_STORED),
                h.ttv_tower_bwd_workspace_bytes_ex(C.byref(d), C.byref(b), _lib.TTV_TAPE_RECOMPUTE))

    off = sizes()
    assert off == sizes() and min(off) > 0
    h.ttv_set_deterministic(1)
    on = sizes()
    assert on == sizes()
    h.ttv_set_deterministic(0)
    assert sizes() == off                           # off again: exactly what it was
    # the partials the backward's reductions need, from the layouts documented in the header: the chain's two gains over L rows, the
    # widest column sum (64 rows per block) and the token-width outer product (32 rows per block)
    L, P, K, dm = b.total_rows, b.sum_patches, b.sum_tokens, d.width
    pd = d.pix_channels * d.patch_t * d.patch_h * d.patch_w
    need = max(2 * h.ttv_rmsnorm_backward_det_scratch_bytes(r, dm) for r in (L, P, K))
    need = max(need, h.ttv_colsum_det_scratch_bytes(L, max(dm, pd)), h.ttv_outer_small_det_scratch_bytes(K, d.token_size, dm))
    for a, o in zip(on, off):
        assert o + need <= a <= o + need + 256      # one more 256-byte aligned region


def test_documented_partial_layouts_give_the_sizes(handle):
    h = handle
    # RMSNorm backward: [blocks][width] fp32, rows dealt over blocks of 4 waves x rows_per_wave, rows_per_wave = ceil(rows / 2048)
    for rows, width in [(9, 256), (300, 320), (2048, 256), (2049, 256), (36864, 1024)]:
        rpw = max(1, -(-rows // 2048))
        blocks = -(-rows // (4 * rpw))
        assert h.ttv_rmsnorm_backward_det_scratch_bytes(rows, width) == blocks * width * 4
        assert h.ttv_rmsnorm_backward_chain_det_scratch_bytes(rows, width) == 2 * blocks * width * 4
    assert h.ttv_colsum_det_scratch_bytes(200, 320) == 4 * 320 * 4
    assert h.ttv_sumall_det_scratch_bytes(3, 200) == 3 * 4
    assert h.ttv_sumall_det_scratch_bytes(36864, 256) == 1024 * 4
    assert h.ttv_outer_small_det_scratch_bytes(300, 5, 256) == 10 * 5 * 256 * 4
    assert h.ttv_outer_small_det_scratch_bytes(300, 64, 256) == 10 * 8 * 256 * 4     # chunks of TTV_MAX_FSQ columns reuse it
    sizes = (C.c_int32 * 3)(5000, 4099, 17)
    assert h.ttv_l1_loss_det_scratch_bytes(sizes, 3) == 3 * 3 * 4                    # ceil(5000 / 2048) = 3 blocks per clip
    assert h.ttv_sq_err_accumulate_det_scratch_bytes(sizes, 3) == 3 * 3 * 16
    assert h.ttv_vq_lookup_backward_det_scratch_bytes(300, 16, 5) == 0               # owner per entry: no partials


def test_size_functions_refuse_bad_input(handle):
    h = handle
    bad = [(h.ttv_rmsnorm_backward_det_scratch_bytes, (-1, 256)), (h.ttv_rmsnorm_backward_det_scratch_bytes, (8, 258)),
           (h.ttv_rmsnorm_backward_det_scratch_bytes, (8, 2048)), (h.ttv_rmsnorm_backward_chain_det_scratch_bytes, (8, 0)),
           (h.ttv_colsum_det_scratch_bytes, (-1, 4)), (h.ttv_colsum_det_scratch_bytes, (4, 0)), (h.ttv_sumall_det_scratch_bytes, (4, 0)),
           (h.ttv_outer_small_det_scratch_bytes, (4, 65, 256)), (h.ttv_outer_small_det_scratch_bytes, (4, 5, 0)),
           (h.ttv_vq_lookup_backward_det_scratch_bytes, (4, 0, 5)), (h.ttv_vq_lookup_backward_det_scratch_bytes, (4, 16, 0)),
           (h.ttv_l1_loss_det_scratch_bytes, (None, 3)), (h.ttv_sq_err_accumulate_det_scratch_bytes, (None, 3)),
           (h.ttv_l1_loss_det_scratch_bytes, ((C.c_int32 * 2)(5, 0), 2)), (h.ttv_sq_err_accumulate_det_scratch_bytes, ((C.c_int32 * 2)(5, -3), 2)),
           (h.ttv_l1_loss_det_scratch_bytes, ((C.c_int32 * 1)(5), -1))]
    for fn, args in bad:
        assert fn(*args) == -1, (fn.__name__, args)
        assert h.ttv_error_string() != b""
    d = _lib.TowerDims()
    assert h.ttv_tower_bwd_workspace_bytes_ex(C.byref(d), None, 0) == -1
