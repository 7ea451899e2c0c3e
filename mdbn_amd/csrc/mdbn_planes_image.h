// LDS image of a 64-deep stage of the narrow (128 x 64) one-plane forward kernel (mdbn_planes.hip, KD = 64), as pure
// functions the host can include: what the loader waves write where, and where the MFMA waves read it back.
// tests/test_narrow_deep_image.py builds a host program from this header and proves that every (row, k-octet) is read from
// where it was written, that every loader instruction copies eight whole 128-byte lines, and that every fragment read is
// free of bank conflicts.
//
//   A     (0/1 sample plane)  [128 rows][64 k] bf16, 128-byte rows, 16 KB at byte 0
//   W p   (plane p = 0..2)    [ 64 rows][64 k] bf16, 128-byte rows,  8 KB at byte 16384 + 8192 p
// 40 KB of a 48-KB ring slot.  The 16-byte chunk c (0..7: k-octet c of the stage) of row r lives at chunk c ^ swz(r).
#pragma once

#if defined(__HIPCC__)
#define MDBN_IMG_FN __host__ __device__ inline
#else
#define MDBN_IMG_FN inline
#endif

namespace mdbn {
namespace deep_image {

constexpr int KD = 64;                         // reduction depth of a stage
constexpr int ROW_BYTES = 2 * KD;              // 128: one cache line
constexpr int A_ROWS = 128, W_ROWS = 64, W_PLANES = 3;
constexpr int A_BYTES = A_ROWS * ROW_BYTES, W_BYTES = W_ROWS * ROW_BYTES;
constexpr int STAGE_BYTES = A_BYTES + W_PLANES * W_BYTES;          // 40960
constexpr int INSTR_ROWS = 8, INSTR_BYTES = INSTR_ROWS * ROW_BYTES;       // one LDS-DMA instruction: 64 lanes x 16 bytes
constexpr int A_INSTR = A_ROWS / INSTR_ROWS, W_INSTR = W_ROWS / INSTR_ROWS;
constexpr int NQ = A_INSTR + W_PLANES * W_INSTR;                   // 40 instructions per stage

// (r >> 1) & 7: the 16 rows of a fragment read take every value twice, and the two rows that share one sit in different
// halves of the 64 banks (row * 128 bytes: odd rows begin at bank 32).  (r >> 2) & 7 would be 4-way conflicted.
MDBN_IMG_FN int swz(int row) { return (row >> 1) & 7; }

// byte offset of a plane image inside the stage: A (plane ignored) or W plane p
MDBN_IMG_FN int plane_base(bool is_a, int plane) { return is_a ? 0 : A_BYTES + plane * W_BYTES; }

// ---- loader: instruction q (0..NQ-1) of a stage, lane 0..63
struct Piece {
    bool is_a;          // operand
    int plane;          // W plane (0 for A)
    int row;            // row of the tile (A: 0..127, W: 0..63)
    int src_chunk;      // 16-byte chunk of the row's 128 source bytes this lane fetches
    int lds;            // byte of the stage it lands at
};
// LDS-DMA writes linearly: wave base + 16 * lane
MDBN_IMG_FN int instr_base(int q)
{
    return q < A_INSTR ? q * INSTR_BYTES : plane_base(false, (q - A_INSTR) / W_INSTR) + ((q - A_INSTR) % W_INSTR) * INSTR_BYTES;
}
MDBN_IMG_FN Piece loader_piece(int q, int lane)
{
    Piece p;
    p.is_a = q < A_INSTR;
    p.plane = p.is_a ? 0 : (q - A_INSTR) / W_INSTR;
    const int sub = p.is_a ? q : (q - A_INSTR) % W_INSTR;
    p.row = INSTR_ROWS * sub + (lane >> 3);
    p.src_chunk = (lane & 7) ^ swz(p.row);
    p.lds = instr_base(q) + 16 * lane;
    return p;
}

// ---- MFMA waves: the v_mfma_f32_16x16x32_bf16 fragment of 16-row block `row0`, k-half kh (0 | 1) of the stage: lane reads
// the 16 bytes of row row0 + (lane & 15), k-octet 4 kh + (lane >> 4).  Byte offset inside the plane image.
MDBN_IMG_FN int frag_offset(int row0, int kh, int lane)
{
    const int row = row0 + (lane & 15), c = 4 * kh + (lane >> 4);
    return row * ROW_BYTES + ((c ^ swz(row)) << 4);
}

}  // namespace deep_image
}  // namespace mdbn
