// The tile shapes of the implicit-GEMM engines and the im2col engine's choice among them. Host code, no HIP: pa_kernels.h and
// conv_rows.h include it, and so does engine_plan.h, which has to compile with the host compiler alone.
#pragma once

namespace pa {

// BM x BN (x BK; 32 unless named)
enum GemmTile { TILE_128x128 = 0, TILE_128x64 = 1, TILE_64x64 = 2, TILE_128x64_K64 = 3, TILE_64x64_K64 = 4,
                TILE_256x128 = 5 /* igemm_bf16.hip only */ };

// im2col engine (igemm.hip): the largest tile shape that still gives the chip ~two workgroups per CU (512 tiles)
inline GemmTile im2col_tile(long long M, int N) {
    const long long t128 = (M + 127) / 128 * (N / 64);   // 128 x 64 tiles; half as many 128 x 128 ones
    return (N % 128 == 0 && t128 / 2 >= 512) ? TILE_128x128 : (t128 >= 512 ? TILE_128x64 : TILE_64x64);
}

}  // namespace pa
