"""GPU test: speculation trees over a KV cache through the C ABI of include/mfa_tree.h (the treeMasks= / treeBatchStride= keywords of
AttentionDecode, AttentionDecodeFP8 and AttentionPrefill).

The caches, the poison, the launch and the check are tests/cache_kit.py's.  Sequences (n, qn) = (700, 40), (191, 64) -- P = 127: key P
ends a tile --, (70, 33) -- the tree straddles key 64 --, (5, 5) -- P = 0 --, (0, 3), (1500, 64) and (40, 64) -- n < qn -- in caches of
1536 keys, prefill rows 64; decode takes the same lengths with (G, R) = (8, 4), (1, 32), (8, 1).  NaN (16-bit) or 0x7f (e4m3) in every key
and value at or past each length and in every 64-key tile the range functions say is never walked; paged pools of page 16 whose spare
entries name an all-poison page.  Settings (W, S, sink logits): (none, 0, no), (130, 4, yes) and (64, 70, yes) -- W = rows, the boundary,
and the zones touch.  Trees, another for every sequence: random (parent uniform among the earlier nodes), forests (several roots, nodes
that see only themselves), arbitrary bits with j > r and bits past `live` (without a window), and the chain.  Expected values:
tests/tree_model.py on needle queries; every output element and every L of every live row is held to its bounds at tree_model.MARGIN.
Results must be finite, inside the bounds, and byte-identical between the contiguous, the token-major strided and the paged layout and
between one shared tree and per-sequence copies of it; and with the chain mask the tree launch is the sink-family launch BYTE FOR BYTE,
decode single and in pieces and prefill over its extra, fully masked tiles.  Maxima seen on an MI355X: DESIGN.md 4.17."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cache_kit as ck  # noqa: E402
import decode_model as dm  # noqa: E402
import tree_model as tm  # noqa: E402
from cache_kit import dev, poisoned, same, token_major  # noqa: E402
from metal_flash_attention_amd import AttentionPrefill  # noqa: E402

BATCH = ck.Batch(((700, 40), (191, 64), (70, 33), (5, 5), (0, 3), (1500, 64), (40, 64)), 1536, 2, 64)
LENS, QLENS, B, RP, HKV = BATCH.LENS, BATCH.QLENS, BATCH.B, BATCH.RP, BATCH.HKV
SETTINGS = [(0, 0, False), (130, 4, True), (64, 70, True)]      # (W (0: none), S, sink logits)
# (D, dtype, G, decode R, e4m3 cache): every value of every dimension with both caches; decode (G, R) = (8, 4), (1, 32), (8, 1)
VARIANTS = [(64, torch.bfloat16, 8, 4, False), (128, torch.float16, 1, 32, False), (256, torch.bfloat16, 8, 1, True),
            (256, torch.float16, 8, 4, False), (64, torch.float16, 1, 32, True), (128, torch.bfloat16, 8, 4, True)]
MAKERS = {"random": tm.random_tree, "forest": lambda R, rng: tm.forest(R, rng, 0.4), "arbitrary": tm.arbitrary, "chain": lambda R, rng: tm.chain(R)}
# the tree of a (setting, variant): arbitrary bits only without a window; every kind meets decode and prefill, both caches and every D
TREES = [("arbitrary", "random", "arbitrary", "forest", "arbitrary", "random"), ("random", "forest", "random", "forest", "random", "forest"),
         ("forest", "random", "forest", "random", "chain", "forest")]
base = functools.partial(ck.base, BATCH)
SEEN = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    yield
    if SEEN:
        print("\ntree worst err / bound at margin 1:", {k: round(v, 4) for k, v in SEEN.items()})


def qlens_of(kind):
    return None if kind == "decode" else QLENS


def masks_of(tree, R, seed):
    """[B, R] uint64, another tree for every sequence"""
    return tm.per_sequence(MAKERS[tree], B, R, seed)


def dev_masks(masks):
    """uint64 [R] or [B, R] -> the int64 tensor of its bit patterns on the device, and its batch stride"""
    t = torch.from_numpy(np.ascontiguousarray(masks).view(np.int64)).cuda()
    return dict(treeMasks=t, treeBatchStride=t.shape[1] if t.dim() == 2 else 0)


def walked(kind, G, R, W, S):
    """per sequence [C // 64] bool: the tiles a tree launch walks -- decode the sink launch's, prefill the tree range's for every row block"""
    if kind == "decode":
        return ck.walked(BATCH, kind, G, R, W, S)
    tiles = []
    for n, qn in BATCH.SEQS:
        out = np.zeros(BATCH.C // 64, dtype=bool)
        b, _u0, _u1, e, se = AttentionPrefill.treeTileRange(n, min(qn, R), W, S)
        out[:se] = True
        out[b:e] = True
        tiles.append(out)
    return tiles


def launch(kind, q, k, v, G, *, masks=None, W=0, S=0, logits=None, want_pieces=None, **how):
    """masks None: the sink entries (the launch a chain must equal).  In pieces, the launch form must name the tree kernels"""
    named = dict(window=W, sinkTokens=S, sinkLogits=logits)
    form = None
    if masks is not None:
        named.update(dev_masks(masks))
        form = r"attn_decode%st_d%d_.*_pieces \(" % ("8" if k.dtype == torch.float8_e4m3fn else "16", q.shape[-1])
    return ck.launch(BATCH, kind, q, k, v, G, want_pieces=want_pieces, want_form=None if want_pieces is None else form, **named, **how)


@functools.lru_cache(maxsize=None)
def reference(kind, D, dtype, G, R, W, S, with_logits, fp8, tree, pieces=None):
    """(q, sink logits, masks, model, needle info), computed once per case and shared; the model reads the values a cache stands for"""
    k, v, (ks, vs) = base(D, dtype, fp8)
    fmt, Hq = dm.fmt_of(dtype), HKV * G
    sink = ck.sink_logits(Hq, D + G) if with_logits else None
    masks = masks_of(tree, R, D + G + W)
    seen = k.float().numpy().astype(np.float64) * (ks[None, :, None, None] if fp8 else 1.0)
    q64, info = tm.needle_queries(seen, LENS, qlens_of(kind), Hq, G, R, W, S, masks, fmt, pieces=pieces, page=16)
    q = torch.from_numpy(q64).to(dtype)
    assert torch.equal(q.to(torch.float64), torch.from_numpy(q64))
    ref = tm.model(q, k.float(), v.float(), LENS, qlens_of(kind), G, W, S, sink, masks, pieces=pieces, kscale=ks, vscale=vs)
    return q, sink, masks, ref, info


def hold(kind, o, l, ref, dtype, out, info, tag, sink, masks, W, S):
    ck.hold(BATCH, kind, o, l, ref, dtype, out, info, tag, tm, SEEN, tm.blind(masks, LENS, qlens_of(kind), o.shape[2], W, S), sink)


@pytest.mark.parametrize("variant", range(len(VARIANTS)))
@pytest.mark.parametrize("setting", range(len(SETTINGS)))
@pytest.mark.parametrize("kind", ["decode", "prefill"])
def test_parity_with_the_model_on_poisoned_caches(kind, setting, variant):
    (W, S, with_logits), (D, dtype, G, Rd, fp8) = SETTINGS[setting], VARIANTS[variant]
    tree = TREES[setting][variant]
    R = Rd if kind == "decode" else RP
    k, v, scales = base(D, dtype, fp8)
    sd = (dev(scales[0]), dev(scales[1]))
    tiles = walked(kind, G, R, W, S)
    keep = BATCH.keep(tiles=tiles)
    if W == 130:
        assert tiles[0][0] and not tiles[0][1:8].any() and tiles[0][8:11].all()   # n = 700: the sink tile, a poisoned gap, the window from tile 8
    q, sink, masks, ref, info = reference(kind, D, dtype, G, R, W, S, with_logits, fp8, tree)
    tag = "%s %s cache %s tree" % (kind, "e4m3" if fp8 else "16-bit", tree)
    kd, vd = poisoned(k, keep), poisoned(v, keep)
    common = dict(masks=masks, W=W, S=S, logits=dev(sink), scales=sd)
    o, l = launch(kind, q, kd.cuda(), vd.cuda(), G, **common)
    hold(kind, o, l, ref, dtype, dtype, info, tag, sink, masks, W, S)
    o32, l32 = launch(kind, q, kd.cuda(), vd.cuda(), G, out=torch.float32, **common)   # (unsplit: no workspace is offered)
    hold(kind, o32, l32, ref, dtype, torch.float32, info, tag, sink, masks, W, S)
    (kt, strides), (vt, _) = token_major(kd), token_major(vd)
    assert same(launch(kind, q, kt.cuda(), vt.cuda(), G, cache_kw=dict(strides=dict(K=strides, V=strides)), **common), (o, l)), \
        "the token-major strided layout differs from the contiguous launch"
    kp, vp, kw = ck.paged_pool(k, v, 16, keep, seed=setting + 3 * variant)
    assert same(launch(kind, q, kp, vp, G, cache_kw=kw, **common), (o, l)), "paged 16 differs from the contiguous launch"


@pytest.mark.parametrize("case", [(256, torch.bfloat16, 8, 4, False, 0, 6, "arbitrary"), (128, torch.float16, 1, 32, True, 1, 3, "random"),
                                  (64, torch.bfloat16, 8, 1, False, 2, 3, "forest")])
def test_decode_in_pieces(case):
    """with a workspace: no window plans 6 pieces over the 24 tiles of the column, W = 640 plans 3 -- as the sink launch does: the plan
    does not change with a tree.  n = 1500 fills every piece, n = 70 leaves pieces empty, n = 0 all of them"""
    D, dtype, G, R, fp8, setting, pieces, tree = case
    W, S, with_logits = SETTINGS[setting]
    W = 640 if W else 0
    k, v, scales = base(D, dtype, fp8)
    keep = BATCH.keep(tiles=walked("decode", G, R, W, S))
    q, sink, masks, ref, info = reference("decode", D, dtype, G, R, W, S, with_logits, fp8, tree, pieces)
    for out in (None, torch.float32):
        o, l = launch("decode", q, poisoned(k, keep).cuda(), poisoned(v, keep).cuda(), G, masks=masks, W=W, S=S, logits=dev(sink), out=out,
                      workspace=True, want_pieces=pieces, scales=(dev(scales[0]), dev(scales[1])))
        hold("decode", o, l, ref, dtype, out or dtype, info, "decode pieces%s %s tree" % (" e4m3" if fp8 else "", tree), sink, masks, W, S)


@pytest.mark.parametrize("variant", range(len(VARIANTS)))
@pytest.mark.parametrize("kind", ["decode", "prefill"])
def test_one_shared_tree_is_its_per_sequence_copies_byte_for_byte(kind, variant):
    D, dtype, G, Rd, fp8 = VARIANTS[variant]
    W, S, with_logits = SETTINGS[1 + variant % 2]
    R = Rd if kind == "decode" else RP
    k, v, scales = base(D, dtype, fp8)
    sd = (dev(scales[0]), dev(scales[1]))
    keep = BATCH.keep(tiles=walked(kind, G, R, W, S))
    q, sink, _masks, _ref, _info = reference(kind, D, dtype, G, R, W, S, with_logits, fp8, "random")
    one = tm.random_tree(R, np.random.default_rng(variant))
    kd, vd = poisoned(k, keep).cuda(), poisoned(v, keep).cuda()
    shared = launch(kind, q, kd, vd, G, masks=one, W=W, S=S, logits=dev(sink), scales=sd)
    copies = launch(kind, q, kd, vd, G, masks=np.tile(one, (B, 1)), W=W, S=S, logits=dev(sink), scales=sd)
    assert same(shared, copies), "batchStride 0 differs from per-sequence copies of the same tree"


def random_q(Hq, R, D, dtype, seed):
    return (torch.rand(B, Hq, R, D, generator=torch.Generator().manual_seed(seed)) * 2 - 1).to(dtype)


@pytest.mark.parametrize("variant", range(len(VARIANTS)))
@pytest.mark.parametrize("setting", range(len(SETTINGS)))
@pytest.mark.parametrize("kind", ["decode", "decode pieces", "prefill"])
def test_the_chain_mask_is_the_sink_family_launch_byte_for_byte(kind, setting, variant):
    """mask_r = 2^(r + 1) - 1: d_r = r + 1 and, with W >= rows, today's visible set for every (n, qn, W, S), n < qn included.  Decode runs
    the same plan and steps, single and in pieces; the extra tiles a prefill row block walks are fully masked for its rows and change no
    bit (p = 0, the row maximum untouched, +0 added).  A difference here is a finding: the step that differs, not a bound"""
    (W, S, with_logits), (D, dtype, G, Rd, fp8) = SETTINGS[setting], VARIANTS[variant]
    pieces = kind == "decode pieces"
    kind = kind.split()[0]
    R = Rd if kind == "decode" else RP
    if pieces:
        W = 640 if W else 0
    k, v, scales = base(D, dtype, fp8)
    sd = (dev(scales[0]), dev(scales[1]))
    # (the poison of the TREE launch's walk, which holds the sink launch's: every row block walks what the sequence's first and last do)
    keep = BATCH.keep(tiles=walked(kind, G, R, W, S))
    kd, vd = poisoned(k, keep).cuda(), poisoned(v, keep).cuda()
    Hq = HKV * G
    q = random_q(Hq, R, D, dtype, D + G + setting)
    sink = dev(ck.sink_logits(Hq, D + G)) if with_logits else None
    how = dict(W=W, S=S, logits=sink, scales=sd, workspace=pieces)
    want = launch(kind, q, kd, vd, G, **how)
    for masks in (tm.chain(R), tm.chain(R, B)):
        got = launch(kind, q, kd, vd, G, masks=masks, want_pieces=(6 if W == 0 else 3) if pieces else None, **how)
        assert torch.equal(got[1], want[1]), "L differs from the sink-family launch"
        assert torch.equal(got[0].view(torch.int16), want[0].view(torch.int16)), "O differs from the sink-family launch"
    # bits the kernels must ignore change nothing either: at or past `live`, which is at or past every row count
    if R < 64:
        noisy = tm.chain(R, B) | np.uint64(((1 << 64) - 1) ^ ((1 << R) - 1))
        assert same(launch(kind, q, kd, vd, G, masks=noisy, **how), want), "bits at or past the rows reached the result"
