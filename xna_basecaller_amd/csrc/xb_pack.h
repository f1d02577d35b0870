// xb_pack.h -- the weight packer: every form xb_weights_ready uploads a weight tensor in, as plain host arithmetic.  No HIP:
// tools/host_logic_main.cpp and tests/test_pack_host.py check it without a GPU.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace xb {

typedef _Float16 half_t;

// pieces per 32-row block and k-tile of the fragment-major image for a given nsplit (lane l = 32 h + r holds row r):
//   nsplit 1, 2: piece 0, 1: the 8 fp16 `hi` values of columns 32 kt + 16 ks + 8 h .. + 8, ks = 0, 1
//   nsplit 2: pieces 2, 3 = bytes 0..15 / 16..31 of the q8 half the B role reads (h = 0: the l8 codes of the 32 columns, h = 1:
//   the h8 codes)
//   nsplit 3 (16x16x32 fragments): lane l = 16 g + r; piece 2 part + c (part 0 = hi, 1 = lo; c = 0, 1) holds row 16 c + r's eight
//   values of columns 32 kt + 8 g .. + 8
inline int gemm4_pieces(int nsplit) { return nsplit == 1 ? 2 : 4; }

// OCP e4m3 (fn) encoding of x: round to nearest even, saturating at +-448 (the MFMA's operand format on gfx950)
inline uint8_t f32_to_e4m3(float x)
{
    const uint8_t sign = std::signbit(x) ? 0x80 : 0x00;
    const float a = std::fabs(x);
    if (!(a == a)) return sign | 0x7f;
    if (a >= 448.0f) return sign | 0x7e;
    if (a < 0.015625f) {                                   // subnormal: steps of 2^-9
        const int q = (int)std::nearbyint(std::ldexp(a, 9));
        return sign | (uint8_t)q;                          // q == 8 is the smallest normal, encoded 0x08 as well
    }
    int ex;
    (void)std::frexp(a, &ex);                              // a = m * 2^ex, m in [0.5, 1)
    int e = ex - 1;
    int q = (int)std::nearbyint(std::ldexp(a, 3 - e));     // 8 .. 16
    if (q == 16) { q = 8; ++e; }
    const int code = ((e + 7) << 3) | (q - 8);
    return sign | (uint8_t)(code > 0x7e ? 0x7e : code);
}

// rows of `cols` floats -> split fp16 (hi, lo) with leading dimension ld.  q8_exp != nullptr: `lo` receives the q8
// image instead (xb_internal.h): per row and 32 columns [32 x e4m3(hi * 2^e) | 32 x e4m3(lo * 2^(e+11))], e chosen so
// that the largest |value| lands near 224, and *q8_exp = e.
inline void split_rows(const float *src, int rows, int cols, int ld, std::vector<half_t> &hi, std::vector<half_t> &lo,
                       int *q8_exp = nullptr)
{
    hi.assign((size_t)rows * ld, (half_t)0.0f);
    lo.assign((size_t)rows * ld, (half_t)0.0f);
    int e = 0;
    if (q8_exp) {
        float amax = 0.0f;
        for (size_t i = 0; i < (size_t)rows * cols; ++i) amax = std::fmax(amax, std::fabs(src[i]));
        if (amax > 0.0f && std::isfinite(amax)) e = (int)std::floor(std::log2(448.0f / amax)) - 1;
        e = e < -16 ? -16 : (e > 32 ? 32 : e);
        *q8_exp = e;
    }
    uint8_t *q = reinterpret_cast<uint8_t *>(lo.data());
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) {
            const float v = src[(size_t)r * cols + c];
            const half_t h = (half_t)v;
            const float l = v - (float)h;
            hi[(size_t)r * ld + c] = h;
            if (!q8_exp) {
                lo[(size_t)r * ld + c] = (half_t)l;
            } else {
                uint8_t *blk = q + ((size_t)r * ld + (c & ~31)) * 2;
                blk[c & 31] = f32_to_e4m3(std::ldexp((float)h, e));
                blk[32 + (c & 31)] = f32_to_e4m3(std::ldexp(l, e + 11));
            }
        }
}

// Fragment-major image of a GEMM B operand for gemm4p_kernel (layout: xb_internal.h, GemmParams::b4).  `hi` / `lo` are
// split_rows outputs with leading dimension ld (lo = the fp16 residual for nsplit 3, the q8 image for nsplit 2, unused for
// nsplit 1); rows are padded with zeros to a multiple of 256 so that no tile needs a bounds check.
inline void fragment_major(const std::vector<half_t> &hi, const std::vector<half_t> &lo, int rows, int ld, int K, int nsplit,
                           std::vector<unsigned char> &out, size_t *kstride)
{
    const int rows4 = (rows + 255) & ~255, nt32 = rows4 / 32, npc = gemm4_pieces(nsplit), nk = K / 32;
    *kstride = (size_t)nt32 * npc * 1024;
    out.assign((size_t)nk * *kstride, 0);
    const unsigned char *hib = reinterpret_cast<const unsigned char *>(hi.data());
    const unsigned char *lob = reinterpret_cast<const unsigned char *>(lo.data());
    if (nsplit == 3) {
        // the 16x16x32 arithmetic: piece 2 * part + c = rows 16 c .. 16 c + 15 of the block, lane l = row (l & 15), k 8 (l >> 4) .. + 8
        for (int kt = 0; kt < nk; ++kt)
            for (int nt = 0; nt < nt32; ++nt)
                for (int c = 0; c < 2; ++c)
                    for (int l = 0; l < 64; ++l) {
                        const int r = nt * 32 + c * 16 + (l & 15);
                        if (r >= rows) continue;
                        unsigned char *blk = out.data() + (size_t)kt * *kstride + (size_t)nt * npc * 1024 + (size_t)l * 16;
                        const size_t e0 = (size_t)r * ld + (size_t)kt * 32 + (size_t)(l >> 4) * 8;
                        memcpy(blk + c * 1024, hib + e0 * 2, 16);
                        memcpy(blk + (2 + c) * 1024, lob + e0 * 2, 16);
                    }
        return;
    }
    for (int kt = 0; kt < nk; ++kt)
        for (int nt = 0; nt < nt32; ++nt)
            for (int l = 0; l < 64; ++l) {
                const int r = nt * 32 + (l & 31), h = l >> 5;
                if (r >= rows) continue;
                unsigned char *blk = out.data() + (size_t)kt * *kstride + (size_t)nt * npc * 1024 + (size_t)l * 16;
                const size_t e0 = (size_t)r * ld + (size_t)kt * 32;          // element offset of the row's k-tile
                for (int ks = 0; ks < 2; ++ks) memcpy(blk + ks * 1024, hib + (e0 + ks * 16 + h * 8) * 2, 16);
                if (nsplit == 2) {
                    // q8 block of the 32 columns: [h8 x 32 | l8 x 32]; the B role reads l8 in lanes 0-31, h8 in lanes 32-63
                    const unsigned char *q = lob + e0 * 2 + (h == 0 ? 32 : 0);
                    memcpy(blk + 2 * 1024, q, 16);
                    memcpy(blk + 3 * 1024, q + 16, 16);
                }
            }
}

// An LSTM layer's weights and biases (PyTorch layout, gates i,f,g,o) in gate-interleaved row order:
// row' = unit*4 + gate  <-  row = gate*F + unit; the bias is b_ih + b_hh
inline void gate_interleave(const float *wih, const float *whh, const float *bih, const float *bhh, int F,
                            std::vector<float> &wi, std::vector<float> &wh, std::vector<float> &bb)
{
    wi.resize((size_t)4 * F * F); wh.resize((size_t)4 * F * F); bb.resize((size_t)4 * F);
    for (int u = 0; u < F; ++u)
        for (int q = 0; q < 4; ++q) {
            memcpy(&wi[((size_t)u * 4 + q) * F], &wih[((size_t)q * F + u) * F], sizeof(float) * F);
            memcpy(&wh[((size_t)u * 4 + q) * F], &whh[((size_t)q * F + u) * F], sizeof(float) * F);
            bb[(size_t)u * 4 + q] = bih[(size_t)q * F + u] + bhh[(size_t)q * F + u];
        }
}

// int8-limb image: per row q = round(W / s * 32512), s = max |W| of the row; q = 256 d1 + d0 with both digits in
// [-128, 127]; h is published as round(h * 32512) the same way, so W h = s / 32512^2 * sum q_w q_h
inline void i8_limbs(const float *w, int rows, int cols, std::vector<int8_t> &d1, std::vector<int8_t> &d0, std::vector<float> &sc)
{
    d1.resize((size_t)rows * cols); d0.resize((size_t)rows * cols); sc.resize((size_t)rows);
    for (int r = 0; r < rows; ++r) {
        float mx = 0.0f;
        for (int k = 0; k < cols; ++k) mx = std::max(mx, std::fabs(w[(size_t)r * cols + k]));
        const float sr = mx > 0.0f ? mx : 1.0f;
        sc[r] = sr / (32512.0f * 32512.0f);
        for (int k = 0; k < cols; ++k) {
            const int q = (int)std::lrintf(w[(size_t)r * cols + k] / sr * 32512.0f);
            const int lo8 = ((q + 128) & 255) - 128;
            d0[(size_t)r * cols + k] = (int8_t)lo8;
            d1[(size_t)r * cols + k] = (int8_t)((q - lo8) >> 8);
        }
    }
}

}  // namespace xb
