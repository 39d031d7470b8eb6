"""What the n-best edit-distance tests share: the C ABI's host entry on numpy arrays, the two dynamic-programming
references (`pika_amd.mbr.edit_distance`, plain Python, and `pika_edit_distances`, the library's two-row DP), and the
seeded length grid.  Every comparison made with these is exact integer equality.

The grid.  Reference lengths 0, 1, 63, 64, 65, 127, 128, 129, 4096 -- empty, one token, and one below / at / one above
one and two 64-position blocks, and the limit -- crossed with hypothesis lengths 0, 1, 64, 65, 130: empty, one token, one
full chunk of 64 columns, one column into the second chunk, two columns into the third.  Two alphabets: two tokens (ties
everywhere, long runs of matches) and 5000 values spread over all of int32 with -2**31, -1, 0 and 2**31 - 1 among them.
All sequences of one utterance are edited prefixes of one master sequence, so every pair shares long stretches and the
distances are neither 0 nor simply the longer length.  Whatever lies beyond an entry's length is POISON: a token of the
sequence itself (the master's first token for an empty one), which would change the result if it were ever read.
"""
import ctypes

import numpy as np

REF_LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129, 4096)
HYP_LENGTHS = (0, 1, 64, 65, 130)
LA, LR = 130, 4096
ALPHABETS = ("two", "int32")


def pool(alphabet, rng):
    if alphabet == "two":
        return np.array([3, 7], dtype=np.int64)
    values = rng.randint(-2 ** 31, 2 ** 31, size=4996, dtype=np.int64)
    return np.concatenate([values, [-2 ** 31, -1, 0, 2 ** 31 - 1]])


def edited_prefix(master, n, tokens, rng):
    """n tokens: master[:n] after max(1, n // 8) edits, each a substitution or a deletion that pulls the master's next
    token in at the end (the length stays n)."""
    seq = [int(t) for t in master[:n]]
    nxt = n
    for _ in range(max(1, n // 8) if n else 0):
        at = int(rng.randint(0, n))
        if rng.randint(0, 2) and nxt < len(master):
            del seq[at]
            seq.append(int(master[nxt]))
            nxt += 1
        else:
            seq[at] = int(tokens[rng.randint(0, len(tokens))])
    return seq


def pack(rows, width, poison):
    """rows: sequences, None (missing: length -1) or (sequence, stored length) -> (tokens (n,width) i32, lengths i32)."""
    tokens = np.empty((len(rows), width), dtype=np.int32)
    lengths = np.empty(len(rows), dtype=np.int32)
    for k, row in enumerate(rows):
        seq, stored = ([], -1) if row is None else (row if isinstance(row, tuple) else (row, len(row)))
        tokens[k] = seq[len(seq) // 2] if seq else poison
        tokens[k, :len(seq)] = seq
        lengths[k] = stored
    return tokens, lengths


def draw(alphabet, seed, hyp_lengths, ref_lengths):
    """One utterance: (hyps, refs) as lists of token lists with the lengths asked for, and the poison token."""
    rng = np.random.RandomState(seed)
    tokens = pool(alphabet, rng)
    master = tokens[rng.randint(0, len(tokens), size=LR + 64)]
    hyps = [edited_prefix(master, n, tokens, rng) for n in hyp_lengths]
    refs = [edited_prefix(master, n, tokens, rng) for n in ref_lengths]
    return hyps, refs, int(master[0])


def host(a_tokens, a_lengths, r_tokens, r_lengths):
    """pika_ctc_edit_distance_host on numpy arrays (B,Na,La), (B,Na), (B,Nr,Lr), (B,Nr) -> (B,Na,Nr) int32."""
    from pika_amd import _lib
    arrays = [np.ascontiguousarray(x, dtype=np.int32) for x in (a_tokens, a_lengths, r_tokens, r_lengths)]
    (B, Na, La), (_, Nr, Lr) = arrays[0].shape, arrays[2].shape
    assert arrays[1].shape == (B, Na) and arrays[3].shape == (B, Nr) and arrays[2].shape[0] == B
    out = np.full((B, Na, Nr), -77, dtype=np.int32)
    ptr = [ctypes.c_void_p(x.ctypes.data) if x.size else None for x in arrays]
    rc = _lib.lib().pika_ctc_edit_distance_host(ptr[0], ptr[1], Na, La, ptr[2], ptr[3], Nr, Lr, B,
                                                ctypes.c_void_p(out.ctypes.data) if out.size else None)
    assert rc == 0, rc
    return out


def dp(hyps, refs, python_below=130):
    """(Na,Nr) distances of token lists (None: missing, -1) by the library's two-row DP, and by the plain Python DP as
    well wherever the reference is shorter than `python_below`."""
    from pika_amd import mbr
    where = [(i, j) for i, h in enumerate(hyps) for j, r in enumerate(refs) if h is not None and r is not None]
    # the two-row DP takes tokens as int32 too
    got = mbr.edit_distances([(hyps[i], refs[j]) for i, j in where])
    out = np.full((len(hyps), len(refs)), -1, dtype=np.int32)
    for (i, j), d in zip(where, got):
        if len(refs[j]) < python_below:
            assert mbr.edit_distance(hyps[i], refs[j]) == d, (i, j)
        out[i, j] = d
    return out
