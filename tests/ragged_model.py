"""Helpers of the ragged-batch tests (include/mfa_ragged.h; a plain module, numpy only): the packed and the padded layouts of one set of
sequences, and a brute-force slot map written from the rule.  Values come from tests/sink_model.py / tests/prefill_model.py; nothing of
either is repeated here.

  packed layout   q, o [T, heads, D], l [heads, T]; sequence b owns the rows [starts[b], starts[b] + qn_b)
  padded layout   q, o [B, heads, rows, D], l [B, heads, rows]; sequence b uses its first qn_b rows (queryLengths)
"""
import numpy as np

NONE = None   # the sequence of a slot past the last row block


def row_starts(counts):
    """[B + 1] starts of sequences with `counts` rows, packed back to back (the layout has no gaps: a sequence's rows end where the
    next one's start, and rows are left unowned only by the cap or by T)"""
    return [0] + [int(x) for x in np.cumsum([int(c) for c in counts])]


def counts_of(starts, total, cap):
    """[(s_b, qn_b)] from the rule: s_b = min(starts[b], T), e_b = min(starts[b + 1], T), qn_b = min(max(e_b - s_b, 0), cap)"""
    out = []
    for b in range(len(starts) - 1):
        s, e = min(int(starts[b]), int(total)), min(int(starts[b + 1]), int(total))
        out.append((s, min(max(e - s, 0), int(cap))))
    return out


def slot_map(starts, total, cap, RB):
    """the brute-force slot map: [(sequence, firstRow)] of every live row block, sequence by sequence, block by block"""
    return [(b, r0) for b, (_s, qn) in enumerate(counts_of(starts, total, cap)) for r0 in range(0, qn, RB)]


def slots(total, batches, cap, RB):
    """the slot bound of include/mfa_ragged.h, on paper"""
    return min(total // RB + batches, batches * -(-cap // RB))


def pack(padded, starts, total, cap, fill=0):
    """padded [B, H, R, ...] -> packed [T, H, ...] (rows no sequence owns: `fill`)"""
    padded = np.asarray(padded)
    out = np.full((total, padded.shape[1]) + padded.shape[3:], fill, dtype=padded.dtype)
    for b, (s, qn) in enumerate(counts_of(starts, total, cap)):
        out[s:s + qn] = np.moveaxis(padded[b, :, :qn], 0, 1)
    return out


def unpack(packed, starts, total, cap, rows, fill=0):
    """packed [T, H, ...] -> padded [B, H, rows, ...] (rows at or past qn_b: `fill`)"""
    packed = np.asarray(packed)
    B = len(starts) - 1
    out = np.full((B, packed.shape[1], rows) + packed.shape[2:], fill, dtype=packed.dtype)
    for b, (s, qn) in enumerate(counts_of(starts, total, cap)):
        out[b, :, :qn] = np.moveaxis(packed[s:s + qn], 0, 1)
    return out


def unpack_l(packed, starts, total, cap, rows, fill=0):
    """packed L [H, T] -> padded [B, H, rows]"""
    return unpack(np.asarray(packed).T[:, :, None], starts, total, cap, rows, fill)[..., 0]


def owned(starts, total, cap):
    """[T] bool: the packed rows some sequence owns"""
    out = np.zeros(total, dtype=bool)
    for s, qn in counts_of(starts, total, cap):
        out[s:s + qn] = True
    return out
