"""GPU test: grouped-query attention through the C ABI (mfa_launch_params.headsPerKeyValue = G).

Every case runs the three kernels twice on the same values: grouped (K / V of Hkv = Hq / G heads, G > 1) and materialised (K / V
repeated per query head, G = 1), and checks
  - forward O, L and backwardQuery dQ, D bit-identical to the materialised launch (the kernels are the same, only their K / V base
    pointers differ);
  - dK / dV bit-identical to the materialised launch's per-query-head gradients summed in fp32 in order g = 0 .. G-1 whenever those
    are FP32 (every descriptor whose outputs are not stored in the 16-bit type: the slabs hold exactly those values);
  - dense and causal cases against the oracle (tests/harness.py tolerances): one oracle Network per query head with its K / V
    arrays overwritten by its K / V head's, dK / dV the fp64 sum over the group of the oracle's per-head gradients;
  - the K / V / dK / dV heads beyond Hkv -- allocated for Hq heads, filled with a finite canary -- neither read into a result nor
    written (a library that ignored the field would read them in bounds and fail the comparison instead of faulting);
  - a workspace filled with NaN before backwardKeyValue, and two grouped runs bit-identical.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import harness  # noqa: E402
from metal_flash_attention_amd import AttentionDescriptor, AttentionKernel, AttentionKernelType, AttentionOperand, GEMMOperandPrecision  # noqa: E402
from metal_flash_attention_amd.torch_binding import pack_block_mask  # noqa: E402
from oracle import Network, NetworkDescriptor  # noqa: E402

T = AttentionKernelType
Op = AttentionOperand
P = GEMMOperandPrecision
DTYPE = {P.FP32: torch.float32, P.FP16: torch.float16, P.BF16: torch.bfloat16}
BITS = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}
KV_CANARY, GRAD_CANARY = -3.0, 1000.0


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    yield


def _descriptor(storage, R, C, D, transposed_kv=False, outputs16=False):
    d = AttentionDescriptor()
    d.lowPrecisionInputs = storage != "f32"
    d.lowPrecisionIntermediates = False
    d.lowPrecisionInputType = P.BF16 if storage == "bf16" else P.FP16
    d.lowPrecisionOutputs = outputs16
    d.matrixDimensions = (R, C, D)
    d.transposeState = (False, transposed_kv, transposed_kv, False)
    return d


def _inputs(B, Hq, Hkv, R, C, D, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g) * 2 - 1  # noqa: E731
    return {Op.Q: rnd(B, Hq, R, D), Op.K: rnd(B, Hkv, C, D), Op.V: rnd(B, Hkv, C, D), Op.dO: rnd(B, Hq, R, D)}


def _run(desc, x, B, Hq, Hkv, R, C, D, causal=False, lengths=None, mask=None, fwd_workspace=False, repeat=1, mask_strides=(0, 0)):
    """one forward + backwardQuery + backwardKeyValue pass with Hkv declared K / V heads (G = Hq / Hkv) -> (values, launch forms, canary
    intact).  Values are fp32 CPU tensors [B, heads, seq, D] / [B, heads, seq] of what the device stored."""
    G = Hq // Hkv
    prec = desc.memoryPrecisions
    kvT = desc.transposeState[1]
    kernels = {t: AttentionKernel(desc.kernelDescriptor(t)) for t in T}
    dev = "cuda"
    bufs, hs, bs, shapes = {}, {}, {}, {}
    for op in (Op.Q, Op.O, Op.dO, Op.dQ, Op.L, Op.D, Op.K, Op.V, Op.dK, Op.dV):
        kv = op in (Op.K, Op.V, Op.dK, Op.dV)
        seq = C if kv else R
        per_head = seq * (1 if op in (Op.L, Op.D) else D)
        heads = Hkv if kv else Hq
        dtype = DTYPE[P(int(prec[op]))]
        # K / V / dK / dV: room for Hq heads, only the first Hkv per batch entry declared (the rest of the buffer is canary)
        fill = KV_CANARY if op in (Op.K, Op.V) else GRAD_CANARY if op in (Op.dK, Op.dV) else 0.0
        buf = torch.full((B * Hq * per_head,), fill, dtype=dtype, device=dev)
        if op in x:
            v = x[op] if not (kv and kvT) else x[op].transpose(2, 3)
            buf[:B * heads * per_head] = v.contiguous().reshape(-1).to(dev, dtype)
        bufs[op], hs[op], bs[op] = buf, per_head, heads * per_head
        shapes[op] = (B, heads, seq, D) if op not in (Op.L, Op.D) else (B, heads, seq)
    kw = dict(row=R, column=C, heads=Hq, batches=B, headStrides=hs, batchStrides=bs, causal=causal, headsPerKeyValue=G)
    if lengths is not None:
        kw.update(rowLengths=lengths[0].to(dev), columnLengths=lengths[1].to(dev))
    if mask is not None:
        kw.update(blockMask=mask.to(dev), blockMaskWords=int(mask.shape[-1]), blockMaskStrides=mask_strides)
    before = {op: bufs[op].clone() for op in (Op.K, Op.V, Op.dK, Op.dV)}
    forms, runs = {}, []
    for _ in range(repeat):
        for t in T:
            need = kernels[t].workspaceSize(row=R, column=C, heads=Hq, batches=B, headsPerKeyValue=G)
            ws = None
            # (backwardKeyValue: the workspace of grouped launches and of re-layout copies only -- a row-parallel split of the
            # materialised launch would sum its pieces in another order than the grouped launch, which is never split)
            wanted = {T.forward: fwd_workspace or kvT, T.backwardQuery: True, T.backwardKeyValue: G > 1 or kvT}[t]
            if need and wanted:
                ws = torch.full(((need + 3) // 4,), float("nan"), dtype=torch.float32, device=dev)   # poison
            forms[t] = kernels[t].launchForm(bufs, workspace=ws, **{k: v for k, v in kw.items()})
            kernels[t].dispatch(bufs, workspace=ws, **kw)
        torch.cuda.synchronize()
        out = {}
        for op in (Op.O, Op.L, Op.D, Op.dQ, Op.dK, Op.dV):
            n = int(np.prod(shapes[op]))
            raw = bufs[op][:n]
            if op in (Op.dK, Op.dV) and kvT:
                b, h, s, d = shapes[op]
                raw = raw.view(b, h, d, s).transpose(2, 3)
            out[op] = raw.reshape(shapes[op]).cpu()
        runs.append(out)
    intact = {}
    for op in (Op.K, Op.V, Op.dK, Op.dV):
        per_head = C * D
        n = B * Hkv * per_head
        intact[op.name] = bool(torch.equal(bufs[op][n:], before[op][n:]))
    return runs, forms, intact


def _bits_equal(a, b):
    return torch.equal(a.view(BITS[a.dtype]), b.view(BITS[b.dtype])) if a.dtype == b.dtype else False


def _group_sum(x, G):
    """[B, Hq, C, D] fp32 per-query-head values -> [B, Hq / G, C, D], summed in fp32 in order g = 0 .. G-1"""
    B, Hq, C, D = x.shape
    y = x.view(B, Hq // G, G, C, D)
    acc = y[:, :, 0].clone()
    for g in range(1, G):
        acc = acc + y[:, :, g]
    return acc


def _oracle(dev_x, B, Hq, Hkv, R, C, D, causal):
    G = Hq // Hkv
    ref = {k: np.zeros(s, np.float64) for k, s in (("O", (B, Hq, R, D)), ("dQ", (B, Hq, R, D)), ("dK", (B, Hkv, C, D)),
                                                       ("dV", (B, Hkv, C, D)))}
    for b in range(B):
        for h in range(Hq):
            j = h // G
            net = Network(NetworkDescriptor(R, C, D), seed=1)
            net.Q = np.ascontiguousarray(dev_x[Op.Q][b, h].numpy(), np.float32)
            net.K = np.ascontiguousarray(dev_x[Op.K][b, j].numpy(), np.float32)
            net.V = np.ascontiguousarray(dev_x[Op.V][b, j].numpy(), np.float32)
            net.dO = np.ascontiguousarray(dev_x[Op.dO][b, h].numpy(), np.float32)
            net.invalidate()
            r = net.run(backward=True, causal=causal)
            ref["O"][b, h], ref["dQ"][b, h] = r["O"], r["dQ"]
            ref["dK"][b, j] += r["dK"]
            ref["dV"][b, j] += r["dV"]
    return ref


def _stored(x, desc):
    """the inputs as the device stores them, back in fp32"""
    prec = desc.memoryPrecisions
    return {op: x[op].to(DTYPE[P(int(prec[op]))]).float() for op in x}


def _case(storage, D, Hq, G, B=1, R=200, C=264, causal=False, lengths=None, mask=None, transposed_kv=False, outputs16=False,
          oracle=True, fwd_workspace=False, seed=0, expect_split=False, mask_strides=(0, 0)):
    Hkv = Hq // G
    desc = _descriptor(storage, R, C, D, transposed_kv, outputs16)
    x = _inputs(B, Hq, Hkv, R, C, D, seed)
    (got, again), forms, intact = _run(desc, x, B, Hq, Hkv, R, C, D, causal, lengths, mask, fwd_workspace, repeat=2, mask_strides=mask_strides)
    assert forms[T.backwardKeyValue].endswith(" + attn_kv_group_sum x%d" % G), forms[T.backwardKeyValue]
    if expect_split:
        assert "column-parallel" in forms[T.forward], forms[T.forward]
    assert all(intact.values()), intact
    for op in got:
        assert _bits_equal(got[op], again[op]), ("two runs differ", op.name)
    # the same launch on K / V materialised per query head
    xm = dict(x)
    xm[Op.K], xm[Op.V] = (x[op].repeat_interleave(G, dim=1) for op in (Op.K, Op.V))
    (mat,), mforms, _ = _run(desc, xm, B, Hq, Hq, R, C, D, causal, lengths, mask, fwd_workspace, mask_strides=mask_strides)
    assert mforms[T.forward] == forms[T.forward] and mforms[T.backwardQuery] == forms[T.backwardQuery], (mforms, forms)
    for op in (Op.O, Op.L, Op.dQ, Op.D):
        assert _bits_equal(got[op], mat[op]), (op.name, forms, (got[op].float() - mat[op].float()).abs().max())
    exact_grads = got[Op.dK].dtype == torch.float32
    valid = torch.ones(B, 1, C, 1, dtype=torch.bool)   # columns < columnLengths[b]; the padding keeps the caller's values
    if lengths is not None:
        valid = (torch.arange(C)[None, :] < lengths[1][:, None].long()).view(B, 1, C, 1)
    for op in (Op.dK, Op.dV):
        assert bool((got[op].float() == GRAD_CANARY)[~valid.expand_as(got[op])].all()), (op.name, "padding written")
        want = torch.where(valid, _group_sum(mat[op].float(), G), got[op].float())
        if exact_grads:
            assert _bits_equal(got[op], want), (op.name, forms[T.backwardKeyValue], (got[op] - want).abs().max())
        else:   # 16-bit outputs: the materialised per-head values were rounded before the sum, the grouped ones after it
            assert torch.allclose(got[op].float(), want, atol=5e-2 * math.sqrt(G), rtol=2e-2), (op.name, (got[op].float() - want).abs().max())
    if oracle and lengths is None and mask is None:
        ref = _oracle(_stored(x, desc), B, Hq, Hkv, R, C, D, causal)
        tol = harness.TOL_FP32 if storage == "f32" else harness.TOL_MIXED
        for name, op in (("O", Op.O), ("dQ", Op.dQ), ("dK", Op.dK), ("dV", Op.dV)):
            # dK / dV: the sum of G per-head gradients carries G independent per-head errors, ~sqrt(G) times one head's (the
            # bit-exact comparison with the materialised launch above is the tight check)
            t = tol[name] * (math.sqrt(G) if name in ("dK", "dV") else 1)
            nbad, err = harness.check(ref[name], got[op].float().numpy(), t)
            assert nbad == 0, (name, err, t, forms)


# every kernel family: head dimensions x storage types (FP32 where the family has it), G over {2, 4, 7, Hq}, Hq over {8, 28}
HEADS = (32, 64, 128, 160, 256, 320, 384, 400)
MATRIX = []
for i, D in enumerate(HEADS):
    for k, storage in enumerate(("f32", "bf16", "f16")):
        Hq, G = ((8, 2), (28, 7), (8, 4), (28, 28), (8, 8), (28, 4))[(i + k) % 6]
        MATRIX.append((storage, D, Hq, G))


@pytest.mark.parametrize("storage,D,Hq,G", MATRIX)
def test_dense_matches_materialised_and_oracle(storage, D, Hq, G):
    _case(storage, D, Hq, G)


@pytest.mark.parametrize("storage,D,Hq,G", [("bf16", 128, 8, 2), ("f16", 64, 28, 7), ("f32", 128, 8, 4), ("bf16", 256, 28, 28),
                                            ("bf16", 320, 8, 4), ("f32", 400, 8, 2)])
def test_causal(storage, D, Hq, G):
    _case(storage, D, Hq, G, R=200, C=264, causal=True)


@pytest.mark.parametrize("storage,D,Hq,G", [("bf16", 128, 8, 4), ("f16", 256, 28, 7), ("f32", 64, 8, 2), ("bf16", 384, 8, 8)])
def test_per_batch_lengths(storage, D, Hq, G):
    lengths = (torch.tensor([200, 131], dtype=torch.int32), torch.tensor([97, 264], dtype=torch.int32))
    _case(storage, D, Hq, G, B=2, lengths=lengths)


@pytest.mark.parametrize("storage,D,Hq,G", [("bf16", 128, 8, 2), ("f16", 64, 28, 7), ("f32", 128, 8, 4), ("bf16", 256, 8, 8)])
def test_block_mask_with_an_unattended_column_block(storage, D, Hq, G):
    bits = torch.tensor([[True, False, True], [True, False, False]])   # 2 row blocks x 3 column blocks; column block 1 never attended
    _case(storage, D, Hq, G, R=300, C=384, mask=pack_block_mask(bits))


@pytest.mark.parametrize("storage,D", [("bf16", 128), ("f16", 64), ("f32", 128)])
def test_block_mask_per_query_head(storage, D):
    """a mask per QUERY head (blockMaskHeadStride counts query heads, include/mfa.h) and per batch entry, Hq = 4, G = 2: the two query
    heads of one K / V head attend different blocks.  Bit-identical to the materialised launch with the same masks and strides, which
    tests/test_train_parity_mask_gpu.py holds to the per-element bounds; a launch that took head h's mask at h / G would differ."""
    B, Hq, G = 2, 4, 2
    patterns = ([[1, 0, 1], [0, 1, 1]], [[0, 1, 0], [1, 1, 0]], [[1, 1, 0], [0, 0, 1]], [[0, 0, 1], [1, 0, 0]],
                [[1, 0, 0], [0, 1, 0]], [[0, 1, 1], [1, 0, 1]], [[1, 1, 1], [0, 1, 0]], [[0, 1, 0], [0, 0, 1]])
    bits = torch.tensor(patterns, dtype=torch.bool).view(B, Hq, 2, 3)           # 2 row blocks x 3 column blocks, all eight different
    mask = torch.stack([pack_block_mask(m) for m in bits.view(-1, 2, 3)]).view(B, Hq, 2, 1)
    _case(storage, D, Hq, G, B=B, R=300, C=384, mask=mask.reshape(-1, 1), mask_strides=(2, 2 * Hq))
    # (the masks matter: with head 0's mask for every head the result is another one)
    desc = _descriptor(storage, 300, 384, D)
    x = _inputs(B, Hq, Hq // G, 300, 384, D, 0)
    (own,), _f, _i = _run(desc, x, B, Hq, Hq // G, 300, 384, D, mask=mask.reshape(-1, 1), mask_strides=(2, 2 * Hq))
    (shared,), _f, _i = _run(desc, x, B, Hq, Hq // G, 300, 384, D, mask=mask.reshape(-1, 1))
    assert not _bits_equal(own[Op.O], shared[Op.O]) and _bits_equal(own[Op.O][0, 0], shared[Op.O][0, 0])


@pytest.mark.parametrize("storage,D,Hq,G", [("bf16", 128, 8, 2), ("f16", 64, 28, 7), ("bf16", 256, 8, 4), ("f32", 128, 8, 8),
                                            ("bf16", 320, 28, 4)])
def test_transposed_kv_through_the_relayout_workspace(storage, D, Hq, G):
    _case(storage, D, Hq, G, transposed_kv=True)


def test_sixteen_bit_outputs():
    _case("bf16", 128, 8, 4, outputs16=True)
    _case("f16", 64, 28, 7, outputs16=True)


def test_split_forward_one_kv_head():
    _case("bf16", 128, 8, 8, R=2048, C=2048, fwd_workspace=True, oracle=False, expect_split=True)
