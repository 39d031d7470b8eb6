// pika_amd/csrc/ctc_edit_core.h -- the bit-vector edit-distance recurrence that the kernel and the host entry of
// ctc_edit.hip share (not part of the C ABI).  Plain C++: it also compiles without hipcc, for host-only test programs.
//
// Myers' bit-vector algorithm in Hyyro's block formulation, GLOBAL distance (Myers, JACM 46(3) 1999; Hyyro, "Explaining
// and extending the bit-parallel approximate string matching algorithm of Myers", 2001).  The reference r[0..S) is the
// pattern, cut into blocks of 64 positions; column j of the DP matrix D[i][j] = distance(r[0..i), a[0..j)) is held as
// vertical differences: bit i of pv / mv of block w says D[64w+i+1][j] - D[64w+i][j] is +1 / -1.  Column 0 is pv = all
// ones, mv = 0.  One step moves one block from column j-1 to column j:
//   eq        bit i set where r[64w+i] == a[j-1]; zero at positions >= S
//   hp_in/hm_in  1 where the horizontal difference D[64w][j] - D[64w][j-1] ABOVE the block is +1 / -1: what the block
//             above returned for this column; (1, 0) into block 0, the boundary row D[0][j] = j
//   top       the bit at which the horizontal difference BELOW is read: 63, or (S - 1) % 64 in the last block
// Bits flow only upwards in the word (the addition's carries and the left shifts), so whatever the bits at positions >= S
// of the last block hold never reaches a bit below them.
#ifndef PIKA_CTC_EDIT_CORE_H
#define PIKA_CTC_EDIT_CORE_H

#if defined(__HIPCC__)
#define PIKA_EDIT_HD __host__ __device__
#else
#define PIKA_EDIT_HD
#endif

#define PIKA_EDIT_MAX_REF 4096   // 64 blocks of 64 positions: one block's state per lane of a wave

typedef unsigned long long edit_word;

PIKA_EDIT_HD inline void ctc_edit_step(edit_word eq, edit_word &pv, edit_word &mv, edit_word hp_in, edit_word hm_in, int top,
                                       edit_word &hp_out, edit_word &hm_out) {
    const edit_word xv = eq | mv;
    eq |= hm_in;                                        // a -1 from above acts as a match at the block's first row
    const edit_word xh = (((eq & pv) + pv) ^ pv) | eq;
    edit_word ph = mv | ~(xh | pv);
    edit_word mh = pv & xh;
    hp_out = (ph >> top) & 1ull;
    hm_out = (mh >> top) & 1ull;
    ph = (ph << 1) | hp_in;
    mh = (mh << 1) | hm_in;
    pv = mh | ~(xv | ph);
    mv = ph & xv;
}

// the number of blocks of a reference of S >= 0 positions, the valid positions of block w and the bit read in it
PIKA_EDIT_HD inline int ctc_edit_blocks(int S) { return (S + 63) >> 6; }
PIKA_EDIT_HD inline edit_word ctc_edit_valid(int S, int w) {
    const int left = S - 64 * w;
    return left >= 64 ? ~0ull : (left <= 0 ? 0ull : (1ull << left) - 1ull);
}
PIKA_EDIT_HD inline int ctc_edit_top(int S, int w) { return w == ctc_edit_blocks(S) - 1 ? (S - 1) & 63 : 63; }

// an entry's token count from its stored length: below 0 missing (-1), beyond the row width the row width
PIKA_EDIT_HD inline int ctc_edit_length(int stored, int width) { return stored < 0 ? -1 : (stored > width ? width : stored); }

#endif
