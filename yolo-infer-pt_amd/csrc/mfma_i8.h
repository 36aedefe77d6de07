// What the kernels on v_mfma_i32_32x32x32_i8 share (reid.hip's similarity, gallery.hip's search):
// the fragment types, the K-contiguous 16-byte operand load and the C/D lane map.
//
// Both operands are K-contiguous rows, so lane l (r = l & 31, h = l >> 5) loads the 16 bytes
// k0 + 16 h .. of row r of its A tile and of its B tile. Whatever order the instruction gives the
// 16 bytes of the two lane halves inside its K = 32, A and B get the same one, and an integer dot
// product does not depend on the order of its terms. The C/D map is the 32x32 one of every dtype:
// register reg of lane (r, h) holds column r of row tile_row(reg, h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace yh {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

// 16 bytes of an operand row (16-byte aligned), or zeros for a row or a K step that does not exist
__device__ __forceinline__ i32x4 load16(const int8_t* p, bool ok) {
    return ok ? *reinterpret_cast<const i32x4*>(p) : i32x4{0, 0, 0, 0};
}

// the A row, inside its 32 x 32 tile, of accumulator register reg in lane half h
__device__ __forceinline__ constexpr int tile_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

}  // namespace yh
