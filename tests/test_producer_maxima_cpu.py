"""Host-side bookkeeping of the producer-reported operand maxima (ops.amax_note / amax_of): a note belongs to one
tensor object and dies with it, like the gradient hints."""
import gc

import torch


def test_a_noted_maximum_belongs_to_one_tensor_object():
    from pointnet_refine_amd import ops
    ops._X_AMAX.clear()
    t = torch.zeros(4, 8)
    a = torch.ones(1)
    ops.amax_note(t, a)
    assert ops.amax_of(t) is a and ops.amax_of(t) is a          # reading does not consume it
    assert ops.amax_of(t[:2]) is None and ops.amax_of(t.detach()) is None and ops.amax_of(torch.zeros(4, 8)) is None
    ops.amax_note(t, None)                                        # nothing produced: the old note stays
    assert ops.amax_of(t) is a
    del t
    gc.collect()
    assert len(ops._X_AMAX) == 0


def test_the_switch_needs_the_split_fp16_mode_and_a_gpu_tensor():
    from pointnet_refine_amd import _lib, ops
    _lib.build()
    lib = _lib.lib()
    old = lib.prh_get_gemm_mode()
    try:
        for mode in (0, 1, 3, 4):
            assert lib.prh_set_gemm_mode(mode) == 0
            assert ops.producer_maxima_on(True) == (mode == 3)
            assert not ops.producer_maxima_on(False)
        lib.prh_set_gemm_mode(3)
        ops.PRODUCER_MAXIMA = False
        assert not ops.producer_maxima_on(True)
    finally:
        ops.PRODUCER_MAXIMA = True
        lib.prh_set_gemm_mode(old)
