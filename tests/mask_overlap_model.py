"""A CPU model of csrc/mask_overlap.hip's two kernels, step by step: the pack kernel's
bands, its 16-byte items (head, aligned vectors, tail) with their 16-bit patterns, the 64-bit
words assembled from them, the window; the pair kernel's considered pairs, window
intersection and popcount cells.  Addresses are modelled: both mask arrays start 16-byte
aligned, as the entry point requires.

``mistake`` plants one named mistake (tests/test_mask_overlap_cpu.py shows that the case named
for it tells it from the contract):
  "past_w"      the item at the row's end reads its whole 16 bytes, past W
  "last_word"   the window intersection leaves out its last word column
  "and1"        a byte counts as set when its lowest bit is, not when it is non-zero
  "alignment"   every row takes its head from the mask's alignment instead of its own, and the
                vector loads, which ignore the low address bits, read from the wrong place
  "beyond"      the masks at or beyond det_count are packed and counted
"""
import numpy as np

STAGE = 4096
MISTAKES = ("past_w", "last_word", "and1", "alignment", "beyond")


def plan(N, D, G, H, W):
    edges = W % 16 != 0
    words = (W + 63) // 64
    items = 1 + (W + 15) // 16 if edges else W // 16
    band = 1 if items >= STAGE else STAGE // items
    masks = N * (D + G)
    align = lambda x: (x + 255) // 256 * 256                                    # noqa: E731
    return dict(words=words, edges=int(edges), pack_blocks=masks, pair_blocks=N * D,
                workspace=align(align(masks * 8 * 4) + masks * H * words * 8), items=items, band_rows=band,
                bands=(H + band - 1) // band)


def popcount(words):
    return int(np.unpackbits(np.ascontiguousarray(words, np.uint64).view(np.uint8)).sum())


def pack_mask(flat, off, H, W, mistake=None):
    """One pack workgroup: the mask at byte offset `off` of `flat` (whose start is 16-byte aligned and
    which is padded behind its end) -> (words uint64 [H, words], area, (r0, r1, c0, c1))."""
    p = plan(1, 1, 0, H, W)
    edges, items, wpr, band = bool(p["edges"]), p["items"], p["words"], p["band_rows"]
    first = 1 if edges else 0
    words = np.zeros((H, wpr), np.uint64)
    for ya in range(0, H, band):
        rows = min(band, H - ya)
        pat = np.zeros((rows, items), np.uint64)
        heads = np.zeros(rows, np.int64)
        for yr in range(rows):                                                  # step one
            row = off + (ya + yr) * W
            head = min((-(off if mistake == "alignment" else row)) % 16, W) if edges else 0
            heads[yr] = head
            for k in range(items):
                xs, xn = k * 16, 16
                if edges:
                    xs = 0 if k == 0 else head + (k - 1) * 16
                    xn = head if k == 0 else 16
                    if xs + xn > W and not (mistake == "past_w" and k >= first and xs < W):
                        xn = W - xs
                if xn == 16 and k >= first:
                    at = row + xs
                    if mistake == "alignment":
                        at -= at % 16                                           # the load ignores the low bits
                    b = flat[at:at + 16]
                else:
                    b = flat[row + xs:row + xs + max(xn, 0)]
                bit = (b & 1) if mistake == "and1" else (b != 0)
                pat[yr, k] = sum(int(v) << j for j, v in enumerate(bit))
        for yr in range(rows):                                                  # step two
            head = int(heads[yr])
            for w in range(wpr):
                c = 64 * w
                word = int(pat[yr, 0]) if edges and w == 0 else 0
                j = 0 if c <= head else (c - head) // 16
                while j < items - first and head + 16 * j < c + 64:
                    sh = head + 16 * j - c
                    v = int(pat[yr, first + j])
                    word |= (v << sh) & (2 ** 64 - 1) if sh >= 0 else v >> -sh
                    j += 1
                words[ya + yr, w] = word
    nz = words != 0
    if not nz.any():
        return words, 0, (0, 0, 0, 0)
    rr, cc = np.nonzero(nz.any(1))[0], np.nonzero(nz.any(0))[0]
    return words, popcount(words), (int(rr[0]), int(rr[-1]) + 1, int(cc[0]), int(cc[-1]) + 1)


def overlap(det_masks, gt_masks, det_labels=None, det_count=None, gt_labels=None, n_class=None, mistake=None):
    """The two launches -> (inter, det_area, gt_area, cells): cells [N, D, G] is the number of (row, word)
    cells the pair kernel read for the pair (0 for a pair that got its 0 from the windows alone)."""
    N, D, H, W = det_masks.shape
    G = gt_masks.shape[1]
    pad = np.zeros(64, np.uint8)
    dflat = np.concatenate([det_masks.reshape(-1), pad])
    gflat = np.concatenate([gt_masks.reshape(-1), pad])
    inter = np.zeros((N, D, G), np.int32)
    da = np.zeros((N, D), np.int32)
    ga = np.zeros((N, G), np.int32)
    cells = np.zeros((N, D, G), np.int64)
    for n in range(N):
        k = D if det_count is None else int(np.clip(det_count[n], 0, D))
        gts = [pack_mask(gflat, (n * G + g) * H * W, H, W, mistake) for g in range(G)]
        for g in range(G):
            ga[n, g] = gts[g][1]
        for d in range(D):
            if d >= k and mistake != "beyond":
                continue
            a_words, da[n, d], a_win = pack_mask(dflat, (n * D + d) * H * W, H, W, mistake)
            live = d < k
            if det_labels is not None:
                dl = int(det_labels[n, d])
                live = live and 1 <= dl < n_class
            for g in range(G):
                if not live or (det_labels is not None and int(gt_labels[n, g]) != dl):
                    continue
                b_words, _, b_win = gts[g]
                ra, rb = max(a_win[0], b_win[0]), min(a_win[1], b_win[1])
                ca, cb = max(a_win[2], b_win[2]), min(a_win[3], b_win[3])
                if mistake == "last_word":
                    cb -= 1
                if ra < rb and ca < cb:
                    cells[n, d, g] = (rb - ra) * (cb - ca)
                    inter[n, d, g] = popcount(a_words[ra:rb, ca:cb] & b_words[ra:rb, ca:cb])
    return inter, da, ga, cells
