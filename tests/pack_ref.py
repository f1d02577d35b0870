"""What the weight packer (csrc/xb_pack.h) has no restatement for elsewhere: the byte decoder of the e4m3 codes, and the
fragment-major image of a GEMM B operand, restated from the layout comments of GemmParams::b4 (csrc/xb_internal.h) and
gemm4_pieces (csrc/xb_pack.h) -- piece by piece, not from the packer's loops.  The roundings themselves (to_e4m3,
split_rows_exp, to_i8_rows) are tests/encoder_f64.py's."""
import numpy as np


def e4m3_decode(b):
    """OCP e4m3 (fn) bytes -> float64."""
    b = b.astype(np.int64)
    s, e, m = (b >> 7) & 1, (b >> 3) & 15, b & 7
    v = np.where(e == 0, m * 2.0 ** -9, (8 + m) * 2.0 ** (e - 10.0))
    return np.where(s == 1, -v, v)


def pieces(nsplit):
    return 2 if nsplit == 1 else 4


def fragment_major(hi, lo, rows, K, nsplit):
    """hi, lo: (rows, ld >= K) 2-byte elements (lo: the fp16 residual for nsplit 3, the q8 image for nsplit 2, unused for
    nsplit 1) -> (image uint8 [K / 32][rows4 / 32][pieces][64 lanes][16 bytes], k-tile stride in bytes)."""
    hib = np.ascontiguousarray(hi).view(np.uint8).reshape(hi.shape[0], -1)        # a row's bytes: element c at 2 c
    lob = np.ascontiguousarray(lo).view(np.uint8).reshape(lo.shape[0], -1)
    rows4 = -(-rows // 256) * 256                     # rows rounded up to 256, the rows beyond `rows` zero
    npc = pieces(nsplit)
    img = np.zeros((K // 32, rows4 // 32, npc, 64, 16), np.uint8)

    def values(src, r, col):                          # the 8 two-byte values of row r from column col on
        return src[r, 2 * col:2 * col + 16]

    for kt in range(K // 32):
        for blk in range(rows4 // 32):
            for lane in range(64):
                if nsplit == 3:
                    # lane l = 16 g + r; piece 2 part + c (part 0 = hi, 1 = lo; c = 0, 1) holds row 16 c + r's eight values of
                    # columns 32 kt + 8 g .. + 8
                    g, r = divmod(lane, 16)
                    for part, src in enumerate((hib, lob)):
                        for c in range(2):
                            row = 32 * blk + 16 * c + r
                            if row < rows:
                                img[kt, blk, 2 * part + c, lane] = values(src, row, 32 * kt + 8 * g)
                    continue
                # lane l = 32 h + r holds row r; piece 0, 1: the 8 fp16 hi values of columns 32 kt + 16 ks + 8 h .. + 8
                h, r = divmod(lane, 32)
                row = 32 * blk + r
                if row >= rows:
                    continue
                for ks in range(2):
                    img[kt, blk, ks, lane] = values(hib, row, 32 * kt + 16 * ks + 8 * h)
                if nsplit == 2:
                    # pieces 2, 3 = bytes 0..15 / 16..31 of the q8 half the B role reads (h = 0: the l8 codes of the 32 columns,
                    # h = 1: the h8 codes); the q8 block of 32 columns is [32 x h8 | 32 x l8] in the place of their residuals
                    block = lob[row, 64 * kt:64 * kt + 64]
                    half = block[32:] if h == 0 else block[:32]
                    img[kt, blk, 2, lane] = half[:16]
                    img[kt, blk, 3, lane] = half[16:]
    return img, rows4 // 32 * npc * 1024
