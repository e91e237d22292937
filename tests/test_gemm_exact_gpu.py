"""Every launch form of the GEMM operator against exact integer answers (tests/gemm_model.py): gemm_f32mfma, gemm_16 128 x 128,
gemm_16 256 x 256 register-staged and LDS-DMA; both 16-bit types, all four transpose pairs, ragged edges in every position,
K from 0 to three tiles and more, every (C type, loadPreviousC) pair, batches with padded, odd and zero strides, a misaligned base,
and fills that use every significand bit.  A and B are surrounded by NaN, C by canaries.  Every launch first asserts the code
object the library says it would run (mfa_gemm_kernel_launch_form), then compares every logical element and every canary of C bit
for bit: there is no tolerance.  tests/test_gemm_sensitivity.py holds, on the CPU, what these comparisons can see.

One line per launch goes to stdout ("gemm-exact <form> C=<type> prev=<0|1> K=<K> batch=<n> <code object>")."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from metal_flash_attention_amd import GEMMDescriptor, GEMMKernel, GEMMKernelDescriptor, GEMMOperandPrecision as P  # noqa: E402
from tests import gemm_model as gm  # noqa: E402

ITEMS = gm.items()


def _descriptor(case):
    d = GEMMDescriptor()
    d.loadPreviousC = case.load
    d.matrixDimensions = (case.M, case.N, case.K)
    d.memoryPrecisions = (P(case.precA), P(case.precB), P(case.precC))
    d.transposeState = (case.tA, case.tB)
    d.leadingDimensions = case.ld
    d.batchDimension = case.batch
    return d


def _device(bits):
    import torch
    t = torch.from_numpy(bits.view(np.uint8).copy()).cuda()
    assert t.data_ptr() % gm.BASE_ALIGNMENT == 0
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("item", ITEMS, ids=[i[0] for i in ITEMS])
def test_every_launch_is_exact_to_the_bit(item):
    import torch
    name, form = item[0], item[1]
    kernels = {}
    stream = torch.cuda.current_stream().cuda_stream
    ran = 0
    for case in gm.cases_of(name):
        data = gm.build(case)
        d = _descriptor(case)
        if (case.precC, case.big) not in kernels:
            kd = GEMMKernelDescriptor(descriptor=d)
            if case.big:
                kd.blockDimensions = (256, 256, 64)
            kernels[(case.precC, case.big)] = GEMMKernel(kd)
        kernel = kernels[(case.precC, case.big)]
        ta, tb, tc = _device(data.A), _device(data.B), _device(data.C0)
        pa = ta.data_ptr() + case.offA * gm.ELEM_SIZE[case.precA]          # A's element (0, 0); the element in front of it is NaN
        strides = case.bs if case.batch > 1 else None
        got_form = kernel.launch_form(pa, tb, tc, descriptor=d, batchStrides=strides)
        assert got_form == gm.expected_form(case), case.name
        print(f"gemm-exact {gm.form_of(case)} C={gm.PREC_NAME[case.precC]} prev={int(case.load)} K={case.K} batch={case.batch} {got_form}")
        kernel.dispatch(pa, tb, tc, descriptor=d, batchStrides=strides, stream=stream)
        torch.cuda.synchronize()
        report = gm.compare(tc.cpu().numpy().view(gm.STORE_DTYPE[case.precC]), data)
        assert report is None, report
        ran += gm.form_of(case) == form
    assert ran >= 20, (name, ran)       # the item's own form really ran (tests/test_gemm_sensitivity.py holds what it covers)
