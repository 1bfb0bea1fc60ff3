"""CPU checks of the long-sequence attention limits: the entry points validate their arguments before any device work, so the
refusals (beyond 32768 tokens, token counts that are not multiples of 256, head_dim != 64) are testable without a GPU, and the
engines' shape guards refuse buffers whose element offsets would pass 2^31."""

from __future__ import annotations

import ctypes

import pytest

from diffulab_amd import _lib, ops

FAKE = ctypes.c_void_p(256)  # never dereferenced: validation returns first


@pytest.mark.parametrize("Nq,Nk,dh,needle", [(32768 + 256, 4096, 64, "32768"), (4096, 32768 + 256, 64, "32768"),
                                             (4096 + 64, 4096, 64, "multiples of 256"), (4096, 4096, 128, "head_dim 128")])
def test_ex_entry_points_refuse(Nq, Nk, dh, needle):
    L = _lib.lib()
    with pytest.raises(RuntimeError, match="dl_attn_fwd_ex") as e:
        L.call("dl_attn_fwd_ex", FAKE, FAKE, FAKE, FAKE, FAKE, 1, 1, Nq, Nk, dh, ctypes.c_float(0.125), None, None)
    assert needle in str(e.value)
    with pytest.raises(RuntimeError, match="dl_attn_bwd_ex") as e:
        L.call("dl_attn_bwd_ex", FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 1, 1, Nq, Nk, dh, ctypes.c_float(0.125), None, None)
    assert needle in str(e.value)


@pytest.mark.parametrize("N,dh", [(32768 + 256, 64), (2304 + 64, 64), (4096, 128)])
def test_square_entry_points_refuse(N, dh):
    L = _lib.lib()
    for name, nptr in (("dl_attn_fwd", 5), ("dl_attn_bwd", 9)):
        with pytest.raises(RuntimeError, match=name):
            L.call(name, *([FAKE] * nptr), 1, 1, N, dh, ctypes.c_float(0.125), None)


def test_row_extent_guard():
    assert ops.ATTN_MAX_TOKENS == 32768
    ops.check_row_extent(16 * 4608, 5120, "ok")  # the joint txt-to-img shape at 4096 + 300 tokens, batch 16
    with pytest.raises(NotImplementedError, match="2\\^31"):
        ops.check_row_extent(128 * 4608, 5120, "too big")
