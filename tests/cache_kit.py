"""What the GPU tests over the KV cache share (a plain module like harness.py and strided.py: no test, no fixture): the batch as a value,
its caches, the poison that proves a kernel never loads what it must not, one launch on sentinel-filled buffers and one check of the
result.  tests/test_window_gpu.py, test_sink_gpu.py, test_softcap_gpu.py and test_ragged_gpu.py run on these; the runners of
tests/test_prefill_gpu.py that tests/test_d256_gpu.py shares are at the end.  tests/test_cache_kit.py checks the poison on the CPU:
poisoned() and pool_host() need no GPU, paged_pool() only uploads.
"""
import collections
import functools
import re

import numpy as np
import torch

import decode_model as dm
import prefill_model as pm
import ragged_model as rm
import sink_model as sm
from metal_flash_attention_amd import (AttentionDecode, AttentionDecodeFP8, AttentionPrefill, GEMMOperandPrecision as P, KVCacheAppend,
                                       KVCachePrecision)

LOG2E = 1.4426950408889634
FLT_MAX = float(np.finfo(np.float32).max)
PREC = {torch.bfloat16: P.BF16, torch.float16: P.FP16}
SENT_O, SENT_L = -7.25, 12345.5
TILE = 64


class Batch(collections.namedtuple("Batch", "SEQS C HKV RP")):
    """sequences ((n keys, qn rows), ...) in caches of C keys and HKV heads; RP: the rows of a prefill launch"""
    LENS = property(lambda self: [s[0] for s in self.SEQS])
    QLENS = property(lambda self: [s[1] for s in self.SEQS])
    B = property(lambda self: len(self.SEQS))

    def keep(self, firsts=None, tiles=None):
        """[B][C] bool: the keys below each length, from firsts[b] on and inside the 64-key tiles tiles[b] where those are given"""
        cols = np.arange(self.C)
        out = np.stack([cols < n for n in self.LENS])
        if firsts is not None:
            out &= np.stack([cols >= f for f in firsts])
        if tiles is not None:
            out &= np.stack([np.repeat(t, TILE) for t in tiles])
        return out


# the batch of tests/test_sink_gpu.py, on which the soft-cap and the ragged parity cases run too (its seams: that file's text), and its
# variants (D, dtype, G, decode R, e4m3 cache): every value of every dimension with both caches
SINK_BATCH = Batch(((700, 40), (200, 40), (100, 130), (5, 5), (0, 3), (1500, 129)), 1536, 2, 130)
SINK_VARIANTS = [(64, torch.bfloat16, 1, 1, False), (128, torch.float16, 8, 4, False), (128, torch.bfloat16, 8, 1, True), (64, torch.float16, 1, 4, True)]


def lengths(values):
    return torch.tensor(values, dtype=torch.int32, device="cuda")


def dev(x):
    """a numpy array or a CPU tensor (or None) on the device"""
    return None if x is None else (torch.from_numpy(x) if isinstance(x, np.ndarray) else x).cuda()


def dev_scales(scales):
    return tuple(dev(s) for s in scales)


def poison_of(t):
    return 0x7F if t.dtype == torch.float8_e4m3fn else float("nan")


def raw(t):
    return t.view(torch.uint8) if t.dtype == torch.float8_e4m3fn else t


def token_major(t):
    """[B, HKV, C, D] -> the same values in a [B, C, HKV, D] allocation, and the (leadingDimension, headStride, batchStride) of the view"""
    _B, HKV, C, D = t.shape
    return raw(t).permute(0, 2, 1, 3).contiguous().view(t.dtype), (HKV * D, D, C * HKV * D)


def same(a, b):
    """(O, L) pairs, byte for byte"""
    return torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[1], b[1])


@functools.lru_cache(maxsize=None)
def base(batch, D, dtype, fp8, seed=0):
    """k, v [B, HKV, C, D] (CPU) of the 16-bit type or e4m3, every key a value; per-head scales (float32 numpy) for e4m3, else None"""
    g = torch.Generator().manual_seed(seed + D + 7 * fp8)
    rnd = lambda: (torch.rand(batch.B, batch.HKV, batch.C, D, generator=g) * 2 - 1)  # noqa: E731
    if fp8:
        rng = np.random.default_rng(seed + D)
        return (rnd() * 3).to(torch.float8_e4m3fn), (rnd() * 3).to(torch.float8_e4m3fn), (dm.spread_scales(rng, batch.HKV), dm.spread_scales(rng, batch.HKV))
    return rnd().to(dtype), rnd().to(dtype), (None, None)


def walked(batch, kind, G, R, W, S):
    """per sequence [C // 64] bool: the 64-key tiles some workgroup of the sequence walks under window W and S sink tokens (from the
    host's range functions)"""
    tiles = []
    for n, qn in batch.SEQS:
        out = np.zeros(batch.C // TILE, dtype=bool)
        if kind == "decode":
            ranges = AttentionDecode.sinkPieceRange(n, R, W, S, 1, 0)
        else:
            RB, ranges = 128 // G, []
            for r0 in range(0, min(qn, R), RB):
                b, _u0, _u1, e, se = AttentionPrefill.sinkTileRange(n, min(qn, R), r0, RB, W, S)
                ranges += [(0, se * TILE), (b * TILE, e * TILE)]
        for b, e in ranges:
            out[b // TILE:-(-min(e, n) // TILE)] = True
        tiles.append(out)
    return tiles


def sink_logits(Hq, seed=0):
    """one logit per query head, natural units: a share of the softmax mass of the order of the needles'"""
    return np.random.default_rng(40 + seed).uniform(1.0, 4.0, Hq).astype(np.float32)


@functools.lru_cache(maxsize=None)
def sink_reference(batch, kind, D, dtype, G, R, W, S, fp8, with_logits=True, pieces=None, causal=True, qkind="needle"):
    """(q, sink logits, sink_model's model, needle info), computed once per case and shared; the model reads the values a cache stands for"""
    k, v, (ks, vs) = base(batch, D, dtype, fp8)
    fmt, Hq = dm.fmt_of(dtype), batch.HKV * G
    qlens = None if kind == "decode" else batch.QLENS
    sink = sink_logits(Hq, D + G) if with_logits else None
    info = None
    if qkind == "needle":
        seen = k.float().numpy().astype(np.float64) * (ks[None, :, None, None] if fp8 else 1.0)
        q64, info = sm.needle_queries(seen, batch.LENS, qlens, Hq, G, R, W, S, fmt, pieces=pieces, page=16)
        q = torch.from_numpy(q64).to(dtype)
        assert torch.equal(q.to(torch.float64), torch.from_numpy(q64))
    else:
        q = (torch.rand(batch.B, Hq, R, D, generator=torch.Generator().manual_seed(D + G + W)) * 2 - 1).to(dtype)
    ref = sm.model(q, k.float(), v.float(), batch.LENS, qlens, G, W, S, sink, causal=causal, pieces=pieces, kscale=ks, vscale=vs)
    return q, sink, ref, info


def poisoned(t, keep):
    """a copy [B, HKV, C, D] with poison in every key that keep [B][C] does not name"""
    out = raw(t.clone())
    for b in range(t.shape[0]):
        out[b][:, torch.from_numpy(~keep[b])] = poison_of(t)
    return out.view(t.dtype)


def pool_host(k, v, page, keep, seed):
    """(K pool, V pool [pages, HKV, page, D], block table [B, C // page] int32), on the host: shuffled pools that hold the keys keep
    [B][C] names only, poison everywhere else; a table entry whose page holds no such key names the last page of the pool, which is all
    poison"""
    rng = np.random.default_rng(seed)
    B, HKV, C, D = k.shape
    pps = C // page
    spare = B * pps
    perm = rng.permutation(spare)
    pk = raw(torch.empty((spare + 1, HKV, page, D), dtype=k.dtype))
    pk[:] = poison_of(k)
    pv = pk.clone()
    table = np.full((B, pps), spare, dtype=np.int32)
    for b in range(B):
        for i in range(pps):
            held = torch.from_numpy(keep[b, i * page:(i + 1) * page])
            if held.any():
                pg = int(perm[b * pps + i])
                table[b, i] = pg
                pk[pg][:, held] = raw(k)[b, :, i * page:(i + 1) * page][:, held]
                pv[pg][:, held] = raw(v)[b, :, i * page:(i + 1) * page][:, held]
    return pk.view(k.dtype), pv.view(k.dtype), table


def paged_pool(k, v, page, keep, seed):
    """pool_host() on the device, and the launch keywords of the layout"""
    pk, pv, table = pool_host(k, v, page, keep, seed)
    HKV, D = k.shape[1], k.shape[3]
    kw = dict(pageSize=page, blockTable=torch.from_numpy(table).cuda(), blockTableStride=table.shape[1], pageStrides=(HKV * page * D, HKV * page * D),
              strides=dict(K=(D, page * D, 0), V=(D, page * D, 0)))
    return pk.cuda(), pv.cuda(), kw


def launch(batch, kind, q, k, v, G, *, out=None, workspace=False, cache_kw=None, scales=(None, None), want_pieces=None, want_form=None, ragged=None,
           **named):
    """-> (O, L base-2) (CPU) as the launch left them on sentinel-filled buffers; k, v on the device.  `named` goes to the host classes
    as it is (window=, sinkTokens=, sinkLogits=, softcap=, causal=): which of them are PRESENT chooses the C entry.  ragged (row starts,
    T): a prefill whose q is packed [T, Hq, D].  workspace: decode is offered the workspace it asks for; want_pieces is then the piece
    count its size and the launch form must show, want_form a pattern the form must match from its start"""
    Hq, D = q.shape[-3 if ragged is None else -2], q.shape[-1]
    fp8 = k.dtype == torch.float8_e4m3fn
    odt = out or q.dtype
    if ragged is None:
        R = q.shape[2]
        o = torch.full((batch.B, Hq, R, D), SENT_O, dtype=odt, device="cuda")
        l = torch.full((batch.B, Hq, R), SENT_L, dtype=torch.float32, device="cuda")
    else:
        R, T = batch.RP, q.shape[0]
        o = torch.full((T, Hq, D), SENT_O, dtype=odt, device="cuda")
        l = torch.full((Hq, T), SENT_L, dtype=torch.float32, device="cuda")
    kw = dict(cache_kw or {})
    kw.update(rows=R, column=batch.C, heads=Hq, batches=batch.B, headsPerKeyValue=G, causal=True, cacheLengths=lengths(batch.LENS))
    kw.update(named)
    if fp8:
        kw.update(keyScale=scales[0], valueScale=scales[1])
    outp = None if out is None else PREC.get(out, P.FP32)
    if kind == "decode":
        op = (AttentionDecodeFP8 if fp8 else AttentionDecode)(D, PREC[q.dtype], outp)
        if workspace:
            need = op.workspaceSize(**kw)
            if want_pieces is not None:
                assert need == want_pieces * batch.B * Hq * R * (D + 2) * 4
                if want_pieces:
                    form = op.launchForm(workspace=0x1000, workspaceBytes=need, **kw)
                    assert ("x %d pieces" % want_pieces) in form and (want_form is None or re.match(want_form, form)), form
            if need:
                kw.update(workspace=torch.empty(need, dtype=torch.uint8, device="cuda"))
    else:
        op = AttentionPrefill(D, PREC[q.dtype], outp, cachePrecision=KVCachePrecision.E4M3 if fp8 else None)
        if ragged is None:
            kw.update(queryLengths=lengths(batch.QLENS))
        else:
            kw.update(rowStarts=lengths(ragged[0]), totalRows=ragged[1])
    op.dispatch(q.cuda(), k, v, o, l, stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    return o.cpu(), l.cpu()


def sink_blind(W, S, causal=True):
    """the blind-row rule of the sink and soft-cap files: the rows whose frontiers leave no visible key"""
    def rows(b, n, qn):
        lo, lim = sm.frontiers(n, qn, np.arange(qn), W, causal)
        return np.array([sm.visible_keys(int(a), int(e), S).size == 0 for a, e in zip(lo, lim)])
    return rows


def hold(batch, kind, o, l, ref, dtype, out, info, tag, model, seen, blind, sink=None):
    """sentinels kept at and past qn; live rows finite; a live row without a visible key -- blind(b, n, qn) -> bool [qn] or [Hq, qn] --
    holds O = 0 and L = its sink logit (base 2), or -FLT_MAX without logits; every live row inside the bounds of `model` (its compare
    and MARGIN).  seen[tag] keeps the worst err / bound at margin 1"""
    R = o.shape[2]
    for b, (n, qn) in enumerate(batch.SEQS):
        qn = R if kind == "decode" else min(qn, R)
        assert bool((o[b, :, qn:].float() == SENT_O).all()) and bool((l[b, :, qn:] == SENT_L).all()), f"sequence {b}: rows at or past {qn} were written"
        assert bool(torch.isfinite(o[b, :, :qn].float()).all()) and bool(torch.isfinite(l[b, :, :qn]).all()), f"sequence {b}: poison reached a live row"
        dark = torch.from_numpy(np.broadcast_to(blind(b, n, qn), (o.shape[1], qn)).copy())
        assert not o[b, :, :qn][dark].float().any(), f"sequence {b}: a row without a visible key"
        if sink is None:
            assert bool((l[b, :, :qn][dark] == -FLT_MAX).all()), f"sequence {b}: a row without a visible key"
        else:
            want = torch.from_numpy(sink)[:, None].expand(-1, qn)[dark] * np.float32(LOG2E)
            assert torch.allclose(l[b, :, :qn][dark], want, rtol=1e-6, atol=0), f"sequence {b}: a row without a visible key must hold L = its sink logit"
    fmt = dm.fmt_of(dtype)
    qlens = None if kind == "decode" else batch.QLENS
    wo, wl, text = model.compare(o, l / LOG2E, ref, fmt, "f32" if out == torch.float32 else fmt, batch.LENS, qlens, margin=1, info=info)
    seen[tag] = max(seen.get(tag, 0.0), wo, wl)
    print("%s: worst |dO| / bound %.3f, |dL| / bound %.3f at margin 1" % (tag, wo, wl))
    assert wo <= model.MARGIN and wl <= model.MARGIN, text


# ------------------------------------------------ the ragged append of tests/test_ragged_gpu.py (its batch; D = 256 runs it too)
RAGGED_BATCH = Batch(((700, 40), (200, 17), (65, 1), (0, 0), (30, 16), (10, 33), (0, 3)), 768, 2, None)


def bits(t):
    return t.view(torch.int16) if t.dtype in (torch.bfloat16, torch.float16) else t.view(torch.int32)


def append_case(batch, D, dtype, fp8, paged, seed):
    """(packed sources, lens, starts, cap, sentinel-filled caches, keywords, scales) of a ragged append of the batch's rows, page 16"""
    lens, counts, B, C, HKV, PAGE = batch.LENS, batch.QLENS, batch.B, batch.C, batch.HKV, 16
    starts = rm.row_starts(counts)
    T = starts[-1]
    g = torch.Generator().manual_seed(seed)
    kn, vn = ((torch.rand(T, HKV, D, generator=g) * 6 - 3).to(dtype).cuda() for _ in range(2))
    cdt = torch.uint8 if fp8 else dtype
    sent = 0x5A if fp8 else 3.5
    kw, scales = {}, (None, None)
    if paged:
        pps = C // PAGE
        table = torch.from_numpy(np.random.default_rng(seed).permutation(B * pps).astype(np.int32).reshape(B, pps)).cuda()
        kc, vc = (torch.full((B * pps, HKV, PAGE, D), sent, dtype=cdt, device="cuda") for _ in range(2))
        kw = dict(pageSize=PAGE, blockTable=table, blockTableStride=pps, pageStrides=(HKV * PAGE * D, HKV * PAGE * D),
                  strides=dict(kCache=(D, PAGE * D, 0), vCache=(D, PAGE * D, 0)))
    else:
        kc, vc = (torch.full((B, HKV, C, D), sent, dtype=cdt, device="cuda") for _ in range(2))
        kw = dict(column=C)
    if fp8:
        rng = np.random.default_rng(seed)
        scales = tuple(torch.from_numpy(dm.spread_scales(rng, HKV)).cuda() for _ in range(2))
        kw.update(keyScale=scales[0], valueScale=scales[1])
    return kn, vn, lens, counts, starts, T, kc, vc, kw


def append_is_the_per_sequence_append(batch, D, dtype, fp8, paged):
    """the ragged append of the batch's rows against the padded append, once per sequence: the caches byte for byte"""
    kn, vn, lens, counts, starts, T, kc, vc, kw = append_case(batch, D, dtype, fp8, paged, D + fp8)
    HKV = batch.HKV
    app = KVCacheAppend(D, PREC[dtype], KVCachePrecision.E4M3 if fp8 else None)
    stream = torch.cuda.current_stream().cuda_stream
    want_k, want_v = kc.clone(), vc.clone()
    dlens = lengths(lens)
    for b, qn in enumerate(counts):                   # the launch that exists, once per sequence with batches = 1
        if qn == 0:
            continue
        s = starts[b]
        one = dict(kw)
        ks, vs = kn[s:s + qn].transpose(0, 1).contiguous(), vn[s:s + qn].transpose(0, 1).contiguous()   # [Hkv, qn, D]
        if paged:
            one.update(blockTable=kw["blockTable"][b:])
            app.dispatch(ks, vs, want_k, want_v, stream=stream, rows=qn, heads=HKV, batches=1, cacheLengths=dlens[b:], **one)
        else:
            app.dispatch(ks, vs, want_k[b], want_v[b], stream=stream, rows=qn, heads=HKV, batches=1, cacheLengths=dlens[b:], **one)
    app.dispatch(kn, vn, kc, vc, stream=stream, rows=max(counts), heads=HKV, batches=len(lens), cacheLengths=dlens, rowStarts=lengths(starts),
                 totalRows=T, **kw)
    torch.cuda.synchronize()
    assert torch.equal(bits(kc) if not fp8 else kc, bits(want_k) if not fp8 else want_k), "K cache differs from the per-sequence appends"
    assert torch.equal(bits(vc) if not fp8 else vc, bits(want_v) if not fp8 else want_v), "V cache differs from the per-sequence appends"
    sent = 0x5A if fp8 else 3.5
    assert int((kc != sent).sum()) > 0 and int((want_k != sent).sum()) == int((kc != sent).sum())
    # the cap and T: rows past them are not appended, and the sequence's rows land qn_b below its length, not its full count
    kc2, vc2 = torch.full_like(kc, sent), torch.full_like(vc, sent)
    cap = 20
    app.dispatch(kn, vn, kc2, vc2, stream=stream, rows=cap, heads=HKV, batches=len(lens), cacheLengths=dlens, rowStarts=lengths(starts),
                 totalRows=starts[-2] + 1, **kw)
    torch.cuda.synchronize()
    written = sum(min(n, qn) for n, (_s, qn) in zip(lens, rm.counts_of(starts, starts[-2] + 1, cap)))   # (keys below 0 are dropped)
    assert int((kc2 != sent).any(dim=-1).sum()) == written * HKV


# ------------------------------------------------------- the runners of tests/test_prefill_gpu.py (its batch; D = 256 runs on them too)
def strides_of(t):
    return (int(t.stride(2)), int(t.stride(1)), int(t.stride(0)))


def prefill_launch(q, k, v, G, causal, *, lens, qlens, out=None, cache_kw=None, q_strided=False, fp8=False, scales=(None, None)):
    """-> (O [B, Hq, R, D], L [B, Hq, R] base-2) as the launch left them on sentinel-filled buffers"""
    Bq, Hq, Rq, D = q.shape
    pre = AttentionPrefill(D, PREC[q.dtype], out and PREC.get(out, P.FP32), cachePrecision=KVCachePrecision.E4M3 if fp8 else None)
    odt = out or q.dtype
    qd = dev(q)
    strides = {}
    if q_strided:   # rows D + 8 apart, heads and batches padded: the operand is a window of a larger allocation
        buf = torch.full((Bq, Hq + 1, Rq + 3, D + 8), float("nan"), dtype=q.dtype, device="cuda")
        buf[:, :Hq, :Rq, :D] = qd
        qd = buf[:, :Hq, :Rq, :D]
        obuf = torch.full((Bq, Hq + 2, Rq + 1, D + 4), SENT_O, dtype=odt, device="cuda")
        o = obuf[:, :Hq, :Rq, :D]
        strides.update(Q=strides_of(qd), O=strides_of(o))
    else:
        obuf = o = torch.full((Bq, Hq, Rq, D), SENT_O, dtype=odt, device="cuda")
    l = torch.full((Bq, Hq, Rq), SENT_L, dtype=torch.float32, device="cuda")
    kw = dict(cache_kw or {})
    strides.update(kw.pop("strides", {}))
    column = kw.pop("column", k.shape[2])
    if fp8:
        kw.update(keyScale=scales[0], valueScale=scales[1])
    pre.dispatch(qd, k, v, o, l, rows=Rq, column=column, heads=Hq, batches=Bq, headsPerKeyValue=G, causal=causal,
                 cacheLengths=lengths(lens), queryLengths=None if qlens is None else lengths(qlens), strides=strides,
                 stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    if q_strided:
        inside = torch.zeros_like(obuf, dtype=torch.bool)
        inside[:, :Hq, :Rq, :D] = True
        assert bool((obuf[~inside] == SENT_O).all()), "the launch wrote outside O's window"
    return o.cpu(), l.cpu()


def check_dead_and_empty(o, l, lens, qlens):
    """rows at or past qn keep the sentinel bit for bit; live rows of an empty sequence hold O = 0, L = -FLT_MAX; no live NaN"""
    for b, (qn, n) in enumerate(zip(qlens, lens)):
        qn = min(qn, o.shape[2])
        assert bool((o[b, :, qn:].float() == SENT_O).all()) and bool((l[b, :, qn:] == SENT_L).all()), f"sequence {b}: rows at or past {qn} were written"
        assert bool(torch.isfinite(o[b, :, :qn].float()).all()) and bool(torch.isfinite(l[b, :, :qn]).all()), f"sequence {b}: poison reached a live row"
        if n == 0:
            assert not o[b, :, :qn].float().any() and bool((l[b, :, :qn] == -FLT_MAX).all()), f"sequence {b}: empty"


def prefill_hold(o, l, ref, dtype, out, info, tag, lens, qlens, seen):
    fmt = dm.fmt_of(dtype)
    outf = "f32" if out == torch.float32 else fmt
    wo, wl, text = pm.compare(o, l / LOG2E, ref, fmt, outf, lens, qlens, margin=1, info=info)
    seen[tag] = max(seen.get(tag, 0.0), wo, wl)
    print("%s: worst |dO| / bound %.3f, |dL| / bound %.3f at margin 1" % (tag, wo, wl))
    assert wo <= pm.MARGIN and wl <= pm.MARGIN, text


def prefill_pool(k, v, page, lens, seed, poison):
    """a shuffled pool [pages, HKV, page, D] holding keys < n only (the rest poison), three pages nobody names, and the table with
    garbage past the last page"""
    rng = np.random.default_rng(seed)
    Bk, Hkv, Ck, D = k.shape
    pps = -(-Ck // page)
    total = Bk * pps + 3
    perm = rng.permutation(total)
    pk = torch.full((total, Hkv, page, D), poison, dtype=k.dtype)
    pv = pk.clone()
    table = np.full((Bk, pps + 2), -7, dtype=np.int32)
    table[:, 1::2] = 2 ** 30
    for b, n in enumerate(lens):
        for i in range(-(-n // page)):
            pg, cnt = int(perm[b * pps + i]), min(page, n - i * page)
            table[b, i] = pg
            pk[pg, :, :cnt] = k[b, :, i * page:i * page + cnt]
            pv[pg, :, :cnt] = v[b, :, i * page:i * page + cnt]
    kw = dict(pageSize=page, blockTable=torch.from_numpy(table).cuda(), blockTableStride=table.shape[1],
              pageStrides=(Hkv * page * D, Hkv * page * D), strides=dict(K=(D, page * D, 0), V=(D, page * D, 0)), column=pps * page)
    return pk.cuda(), pv.cuda(), kw
