"""GPU test: the speculative loop append -> verify -> accept -> continue through the torch binding, at a gpt-oss-like shape kept small
(Hq 8 / Hkv 2, B = 2, prefixes of 70 and 5 keys; D = 64 and 128, each over a bf16 contiguous and an e4m3 paged cache, and D = 256
bf16).  Four steps: a random tree of 12 nodes (prefill) or 4 (decode) is appended and verified by the tree launch, a random leaf per sequence is accepted, tree_path and kv_cache_compact move its path to the front, one more
token is appended under the returned lengths and flash_decode runs.  Beside it a SCRATCH cache receives only the accepted tokens and the
extra one through the append launches.  After every step the two caches agree byte for byte on the slots below the length, and the two
decode outputs and L agree under torch.equal: the kernel, the visible bytes and the lengths are the same, so nothing looser is needed.
Then: the public function against the C-ABI launch and the model byte for byte, and a call captured in a torch.cuda.graph, replayed."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cache_kit as ck  # noqa: E402
import compact_model as cm  # noqa: E402
import tree_model as tm  # noqa: E402
from metal_flash_attention_amd import GEMMOperandPrecision as P, KVCacheCompact, KVCachePrecision  # noqa: E402
from metal_flash_attention_amd import torch_binding as tb  # noqa: E402

HQ, HKV, B, C, PAGE = 8, 2, 2, 128, 16
PREFIX = (70, 5)
STEPS = 4


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


class Cache:
    """a K / V cache pair on the device, contiguous [B, Hkv, C, D] or a shuffled pool [pages, Hkv, 16, D] with its table"""

    def __init__(self, D, dtype, paged, seed):
        fill = lambda shape: torch.full(shape, 0x5A, dtype=torch.uint8, device="cuda")   # noqa: E731
        item = 1 if dtype == torch.float8_e4m3fn else 2
        if paged:
            pps = C // PAGE
            self.table = torch.from_numpy(np.random.default_rng(seed).permutation(B * pps).astype(np.int32).reshape(B, pps)).cuda()
            shape = (B * pps, HKV, PAGE, D)
        else:
            self.table, shape = None, (B, HKV, C, D)
        self.k, self.v = (fill(shape + (item,)).view(dtype).view(shape) for _ in range(2))

    def keys(self, t, b, n):
        """the first n keys of sequence b, [Hkv, n, D] as bytes"""
        raw = t.view(torch.uint8)
        if self.table is None:
            return raw[b, :, :n].cpu()
        pages = self.table[b].long()
        return raw[pages].permute(1, 0, 2, 3).reshape(HKV, C, -1)[:, :n].cpu()


def rnd(g, *shape):
    return (torch.rand(*shape, generator=g) * 2 - 1).bfloat16().cuda()


@pytest.mark.parametrize("D,fp8,paged,kind,R", [(D, fp8, fp8, kind, R) for D in (64, 128) for fp8 in (False, True) for kind, R in (("prefill", 12), ("decode", 4))]
                         + [(256, False, False, "prefill", 12)])
def test_four_speculative_steps_leave_the_cache_a_scratch_cache_would_hold(D, fp8, paged, kind, R):
    g = torch.Generator().manual_seed(D + R)
    rng = np.random.default_rng(D + R)
    dtype = torch.float8_e4m3fn if fp8 else torch.bfloat16
    main, scratch = Cache(D, dtype, paged, 1), Cache(D, dtype, paged, 2)       # (other pages for the same keys)
    scales = dict(k_scale=torch.tensor([0.5, 1.25], device="cuda"), v_scale=torch.tensor([2.0, 0.75], device="cuda")) if fp8 else {}
    host = list(PREFIX)                                                          # the lengths, tracked on the host for the scratch cache
    lens = ck.lengths(host)
    k0, v0 = rnd(g, B, HKV, max(PREFIX), D), rnd(g, B, HKV, max(PREFIX), D)     # (a shorter prefix keeps its last rows: the rest fall before key 0)
    for cache in (main, scratch):
        tb.kv_cache_append(k0, v0, cache.k, cache.v, lens, block_table=cache.table, **scales)
    fn = tb.flash_decode if kind == "decode" else tb.flash_prefill
    for step in range(STEPS):
        masks = tm.per_sequence(tm.random_tree, B, R, 31 * step + D)
        bits = torch.from_numpy(np.array([[[(int(masks[b, r]) >> j) & 1 for j in range(R)] for r in range(R)] for b in range(B)], dtype=bool)).cuda()
        k_new, v_new, q = rnd(g, B, HKV, R, D), rnd(g, B, HKV, R, D), rnd(g, B, HQ, R, D)
        with_tree = lens + R
        tb.kv_cache_append(k_new, v_new, main.k, main.v, with_tree, block_table=main.table, **scales)
        o = fn(q, main.k, main.v, with_tree, block_table=main.table, tree_mask=tb.pack_tree_mask(bits), **scales)
        assert bool(torch.isfinite(o.float()).all())
        leaves = [[r for r in range(R) if not any(int(masks[b, s]) >> r & 1 for s in range(R) if s != r)] for b in range(B)]
        leaf = [int(rng.choice(leaves[b])) for b in range(B)]
        accepted, counts = tb.tree_path(bits, torch.tensor(leaf, device="cuda"))
        paths = [[j for j in range(R) if int(masks[b, leaf[b]]) >> j & 1] for b in range(B)]   # (random_tree: a parent has the smaller index)
        assert accepted.shape == (B, R) and [accepted[b, :len(paths[b])].tolist() for b in range(B)] == paths and counts.tolist() == [len(p) for p in paths]
        new_lens = tb.kv_cache_compact(main.k, main.v, with_tree, accepted, counts, R, block_table=main.table)
        # the scratch cache: only the accepted tokens, packed, through the ragged append
        starts = [0, len(paths[0]), len(paths[0]) + len(paths[1])]
        k_acc = torch.cat([k_new[b][:, paths[b]].transpose(0, 1) for b in range(B)]).contiguous()    # [T, Hkv, D]
        v_acc = torch.cat([v_new[b][:, paths[b]].transpose(0, 1) for b in range(B)]).contiguous()
        host = [n + len(p) for n, p in zip(host, paths)]
        assert new_lens.dtype == torch.int32 and new_lens.tolist() == host
        tb.kv_cache_append_ragged(k_acc, v_acc, scratch.k, scratch.v, ck.lengths(host), ck.lengths(starts), max(len(p) for p in paths),
                                  block_table=scratch.table, **scales)
        # one more token under the returned lengths, and a decode step
        k1, v1, q1 = rnd(g, B, HKV, 1, D), rnd(g, B, HKV, 1, D), rnd(g, B, HQ, 1, D)
        lens = new_lens + 1
        host = [n + 1 for n in host]
        tb.kv_cache_append(k1, v1, main.k, main.v, lens, block_table=main.table, **scales)
        tb.kv_cache_append(k1, v1, scratch.k, scratch.v, ck.lengths(host), block_table=scratch.table, **scales)
        got = tb.flash_decode(q1, main.k, main.v, lens, block_table=main.table, return_lse=True, **scales)
        want = tb.flash_decode(q1, scratch.k, scratch.v, ck.lengths(host), block_table=scratch.table, return_lse=True, **scales)
        torch.cuda.synchronize()
        for b in range(B):
            for name, a, s in (("K", main.k, scratch.k), ("V", main.v, scratch.v)):
                assert torch.equal(main.keys(a, b, host[b]), scratch.keys(s, b, host[b])), f"step {step}, sequence {b}: {name} differs below the length"
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), f"step {step}: the decode step differs from the scratch cache's"
        assert bool(torch.isfinite(got[0].float()).all())
    assert host[0] > PREFIX[0] + STEPS and host[1] > PREFIX[1] + STEPS


TORCH_TYPE = {"e4m3": torch.float8_e4m3fn, "bf16": torch.bfloat16, "f16": torch.float16}


def tensors_of(index):
    """a case of compact_model.CASES as the public function takes it: typed views [B or pages, Hkv, keys, D] of the model's buffers"""
    (config, path), (k, v, geo, want) = cm.CASES[index], cm.run(cm.CASES[index])
    dtype = TORCH_TYPE[config.element]

    def view(buf):
        t = ck.dev(buf.copy()).view(dtype)
        if config.layout == "token-major":
            return t.view(cm.B, cm.CAPACITY, cm.HKV, config.D).permute(0, 2, 1, 3)
        return t.view((geo.pages, cm.HKV, geo.page, config.D) if geo.page else (cm.B, cm.HKV, cm.CAPACITY, config.D))

    args = dict(cache_lengths=ck.dev(np.asarray(path.lens, dtype=np.uint32).view(np.int32)), accepted=ck.dev(path.accepted),
                accepted_counts=ck.dev(np.asarray(path.counts, dtype=np.uint32).view(np.int32)), rows=path.rows,
                q_lengths=None if path.qlens is None else ck.lengths(path.qlens),
                block_table=ck.dev(np.ascontiguousarray(geo.table)) if geo.page else None)
    return config, geo, view(k), view(v), args, want


def flat(t, config):
    """the bytes of a cache view in the order of its allocation"""
    t = t.permute(0, 2, 1, 3) if config.layout == "token-major" else t
    assert t.is_contiguous()
    return t.view(torch.uint8).reshape(-1).cpu().numpy()


PUBLIC = [i for i, (c, p) in enumerate(cm.CASES) if p.name in ("rotation by one", "indices -1 and live", "per-sequence queryLengths", "a negative table entry",
                                                              "reversal of 64 nodes")]


@pytest.mark.parametrize("index", PUBLIC, ids=[cm.case_id(cm.CASES[i]) for i in PUBLIC])
def test_the_public_function_is_the_c_abi_launch_byte_for_byte(index):
    config, geo, k, v, args, (want_k, want_v, want_new) = tensors_of(index)
    _c, _g, ck_, cv_, _a, _w = tensors_of(index)                                # the same case again, for the C-ABI launch
    new = tb.kv_cache_compact(k, v, **args)
    e = cm.ELEMENT_BYTES[config.element]
    strides = (geo.ld // e, geo.hs // e, 0 if geo.page else geo.outer // e)
    kw = dict(strides=dict(kCache=strides, vCache=strides))
    if geo.page:
        kw.update(pageSize=geo.page, blockTable=args["block_table"], blockTableStride=geo.table.shape[1], pageStrides=(geo.outer // e, geo.outer // e))
    else:
        kw.update(column=geo.column)
    abi_new = torch.full((cm.B,), -1, dtype=torch.int32, device="cuda")
    precision = {"e4m3": KVCachePrecision.E4M3, "bf16": P.BF16, "f16": P.FP16}[config.element]
    KVCacheCompact(config.D, precision).dispatch(ck_, cv_, stream=torch.cuda.current_stream().cuda_stream, rows=args["rows"], heads=cm.HKV, batches=cm.B,
                                                 cacheLengths=args["cache_lengths"], queryLengths=args["q_lengths"], accepted=args["accepted"],
                                                 acceptedCounts=args["accepted_counts"], maxAccepted=args["accepted"].shape[1], newLengths=abi_new, **kw)
    torch.cuda.synchronize()
    assert torch.equal(new, abi_new) and np.array_equal(new.cpu().numpy().view(np.uint32), want_new)
    for got, abi, want in ((k, ck_, want_k), (v, cv_, want_v)):
        assert np.array_equal(flat(got, config), flat(abi, config)), "the public function and the C-ABI launch differ"
        assert np.array_equal(flat(got, config), want), "the public function differs from the model"


def test_a_captured_call_replays_to_the_same_bytes():
    index = next(i for i, (c, p) in enumerate(cm.CASES) if c.D == 128 and c.element == "e4m3" and p.name == "rotation by one")
    config, geo, k, v, args, (want_k, want_v, want_new) = tensors_of(index)
    k0, v0 = k.clone(), v.clone()
    tb.kv_cache_compact(k, v, **args)                                            # (warm-up outside the capture)
    torch.cuda.synchronize()
    k.copy_(k0), v.copy_(v0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        new = tb.kv_cache_compact(k, v, **args)
    for _ in range(2):                                                           # (a rotation: a second replay on the moved rows would show)
        k.copy_(k0), v.copy_(v0)
        new.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(flat(k, config), want_k) and np.array_equal(flat(v, config), want_v)
        assert np.array_equal(new.cpu().numpy().view(np.uint32), want_new)
    # the replay follows the device's arrays: another count, no new capture
    args["accepted_counts"].copy_(torch.tensor([2, 0, 5], dtype=torch.int32))
    k.copy_(k0), v.copy_(v0)
    graph.replay()
    torch.cuda.synchronize()
    path = cm.CASES[index][1]
    again = cm.compact(cm.build(config, path.edit)[0], cm.build(config, path.edit)[1], geo, path.lens, path.rows, path.qlens, path.accepted, (2, 0, 5),
                       path.accepted.shape[1])
    assert np.array_equal(flat(k, config), again[0]) and np.array_equal(flat(v, config), again[1])
    assert np.array_equal(new.cpu().numpy().view(np.uint32), again[2])
