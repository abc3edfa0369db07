/* firedancer_amd/csrc/fd_ed25519_ws.h
 *
 * The verify workspace: one plane per intermediate result, laid out by
 * ws_layout_const for host and device alike.  Every stage header includes
 * this one; it also holds the two integer typedefs they all use.
 *
 * Workspace layout (N = n rounded up to 64; every plane is [element][N] so
 * that the 64 lanes of a wave touch 64 consecutive elements):
 *   dig  : u16    [N][256]     slide digit pairs (a_p = h digit, b_p = s digit) as
 *                              int8 (low, high), contiguous per lane
 *   top  : int32  [N]          highest nonzero digit position (-1 if none)
 *   A    : int32  [30][N]      -A.X, A.Y, -A.T   (A.Z == 1)
 *   R    : int32  [20][N]      R.X, R.Y
 *   Ai   : int32  [N][8][4][12] cached odd multiples of -A, rows [Z,Y-X,Y+X,2dT] of
 *                              10 limbs padded to 12: per-lane contiguous (one ADD gathers
 *                              192 contiguous bytes instead of 40 scattered dwords)
 *   st   : uint32 [3][N]       work statistics (iterations, nnz h, nnz s)
 *   ds   : uint8  [N][2]       decompression status of A / R (0 ok, 1 not on the
 *                              curve); k_dsm turns a failure into -2
 *   tag  : uint64 [N]          dedup tag: the first 8 bytes (little endian) of
 *                              SHA-512(R||A||M), 0 when the s check rejected
 *                              (app/frank/README.md:107-110: verify yields a
 *                              secure hash for dedup at no extra cost)
 */

#ifndef FD_ED25519_WS_H
#define FD_ED25519_WS_H

#include "fd_ed25519_dev.h"
#include "fd_ed25519_kernels.h"

typedef int8_t i8;
typedef uint16_t u16;

/* ------------------------------------------------------------------ */
/* workspace                                                            */

__host__ __device__ constexpr size_t ws_al( size_t x ) { return (x + 255UL) & ~(size_t)255UL; }

/* constexpr so that a kernel with a fixed N (k_tile_persist, N = 64) folds
   every plane offset into an immediate */
__host__ __device__ constexpr ws_layout_t
ws_layout_const( size_t n ) {
  ws_layout_t L = {};
  size_t N = (n + 63UL) & ~(size_t)63UL; if( !N ) N = 64;
  size_t o = 0;
  L.N   = N;
  L.dig = o; o = ws_al( o + 2UL*128UL*N );   /* u16 [N][128] digit events: h [0,64), s [64,128) */
  L.evn = o; o = ws_al( o + 4UL*N );          /* u32 [N]: h event count | s count << 8 */
  L.top = o; o = ws_al( o + 4UL*N );
  L.A   = o; o = ws_al( o + 4UL*30UL*N );
  L.R   = o; o = ws_al( o + 4UL*20UL*N );
  L.Ai  = o; o = ws_al( o + 4UL*384UL*N );
  L.st  = o; o = ws_al( o + 4UL*3UL*N );
  L.tag = o; o = ws_al( o + 8UL*N );
  L.ds  = o; o = ws_al( o + 2UL*N );
  L.init = o; o = ws_al( o + 16UL*N );        /* uint4 [N]: k_dsmp op-stream start (k_ai) */
  L.ctr  = o; o = ws_al( o + 16UL );          /* u32 k_dsmp work counter (zeroed by k_ai) | u32 k_dsmp guard flag */
  L.total = o;
  return L;
}

ws_layout_t
fd_amd_ws_layout( size_t n ) {
  return ws_layout_const( n );
}

#endif /* FD_ED25519_WS_H */
