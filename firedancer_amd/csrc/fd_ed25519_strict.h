/* firedancer_amd/csrc/fd_ed25519_strict.h
 *
 * k_strict: the strict RFC 8032 verdict as an overlay on the reference
 * pipeline (FD_ED25519_AMD_MODE_STRICT, include/fd_ed25519_amd.h).  One
 * launch after the DSM stage (after k_fin on the pooled path) re-decides
 * every verdict from the raw input bytes, the decompression planes and the
 * R' that the DSM kernel parked in the signature's Ai slab; nothing upstream
 * changes, and the default mode never launches it.  The per-signature
 * decision (strict_decide) is shared with the streaming tile, whose strict
 * kernel runs it inside each chunk (fd_ed25519_tile.h).
 *
 * The rule, in this order:
 *   1. s = LE(sig[32:64]) >= L                                    -> -1
 *   2. A = pub or R = sig[0:32]: y = LE(bytes) mod 2^255 >= p, not
 *      on the curve, x = 0 with the sign bit set, or one of the 8
 *      torsion points                                             -> -2
 *   3. R' = [s]B - [h]A differs from R as a point                 -> -3
 *   4. otherwise                                                  ->  0
 * Step 1 is the reference's s check with its early "return 0" window
 * (fd_ed25519_user.c:373-379) turned into a reject: every s in the window
 * is >= 2^252 + 2^128 > L.  Step 2 is byte compares plus the ds flags of
 * the decompression: the torsion points have y in {0, 1, p-1, y8, p-y8}
 * (tools/gen_consts.py torsion_y8), and y in {1, p-1} are the only points
 * with x = 0, so "x = 0 with the sign bit set" needs no test of its own.
 * Step 3 compares values, X' = R.x Z' and Y' = R.y Z' mod p over all 255
 * bits, where the reference compares limbs 0..7 of two separately carried
 * products (the cause of its false rejects).
 */

#ifndef FD_ED25519_STRICT_H
#define FD_ED25519_STRICT_H

#include "fd_ed25519_pool.h"
#include "fd_ed25519_dsm8.h"

/* which DSM kernel parked R' (fd_amd_launch_verify's choice) */
enum { STRICT_DSM = 1, STRICT_DSM4 = 2, STRICT_DSM8 = 3, STRICT_DSMP = 4 };

/* a >= c for 256-bit little-endian word arrays */
FD_DEV bool
ge256( u32 const a[8], u32 const c[8] ) {
  bool ge = true;   /* equal so far */
  _Pragma("unroll") for( int k=0; k<8; k++ ) ge = (a[k] != c[k]) ? (a[k] > c[k]) : ge;   /* higher words override */
  return ge;
}

FD_DEV bool
eq256( u32 const a[8], u32 const c[8] ) {
  u32 d = 0u;
  _Pragma("unroll") for( int k=0; k<8; k++ ) d |= a[k] ^ c[k];
  return d == 0u;
}

/* Step 2's byte part for one encoded point: y >= p (non-canonical) or y
   the y of a torsion point. */
FD_DEV bool
strict_bad_encoding( uint4 lo, uint4 hi ) {
  u32 const y[8]   = { lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w & 0x7fffffffu };
  u32 const p[8]   = { 0xffffffedu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x7fffffffu };
  u32 const pm1[8] = { 0xffffffecu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x7fffffffu };
  u32 const y8[8]  = FD_AMD_Y8_WORDS;
  u32 const y8n[8] = FD_AMD_Y8N_WORDS;
  u32 rest = 0u;
  _Pragma("unroll") for( int k=1; k<8; k++ ) rest |= y[k];
  bool const small = rest == 0u && y[0] <= 1u;   /* y = 0 (order 4), y = 1 (the identity) */
  return ge256( y, p ) || small || eq256( y, pm1 ) || eq256( y, y8 ) || eq256( y, y8n );
}

/* Step 3: (X : Y : Z) == (RX, RY) as points, Z != 0 mod p (it is the Z of a
   point of the complete curve).  The two differences X - RX Z and Y - RY Z
   are tested for zero with fe_isnonzero, i.e. canonicalised by the
   reference's fe_tobytes.  X, Y, Z, RX, RY are outputs of the carry chain
   (or fe_frombytes / a negation of one), so both products take carried
   operands and each difference is one of two carried elements: even
   |limb| <= 2^26, odd <= 2^25 + the second-round carries of limbs 1 and 5,
   inside what fe_tobytes accepts (1.1 * 2^26 / 1.1 * 2^25; it is the class
   the decompression already feeds fe_isnonzero).  The reference's compare
   reads the carried limbs themselves, where limbs 1 and 5 may leave the
   balanced range; here they only enter a sum that is reduced as a whole.
   tests/test_strict_compare_cpu.py restates this sequence on the limb
   model and pins it to value(f) % p == value(g) % p. */
FD_DEV bool
strict_point_eq( fe const & X, fe const & Y, fe const & Z, fe const & RX, fe const & RY ) {
  fe xZ, yZ;
  fe_mul_fold2w( xZ, Z, RX, yZ, Z, RY );
  fe const dx = fe_sub( X, xZ ), dy = fe_sub( Y, yZ );
  return !fe_isnonzero( dx ) && !fe_isnonzero( dy );
}

/* The strict verdict of signature slot i from the reference pipeline's
   verdict `code`: the rule above over the slot's raw bytes (pub + 32 i,
   sig + 64 i: 32- / 64-byte aligned records, as k_prep reads them), its ds
   flags and the R' that DSM kernel `kind` (STRICT_*) parked in its Ai slab.
   The caller leaves alone what the rule does not cover (slots with
   skip[i] != 0, FD_AMD_VERDICT_DEVICE) and stores the result.  Callers:
   k_strict below, and the streaming tile's chunk pipeline (tile_chunk<true>,
   fd_ed25519_tile.h), whose workspace is one wave's N = 64 slice.

   Invariant of step 3: a slab is read only for a signature whose DSM ran.
   A verdict of 0 or -3 is written by a DSM compare alone (k_dsm / k_dsm4 /
   k_dsm8 / k_fin, each for a signature that was pending and decodable, so
   its loop ran and parked R'), with one exception: k_prep's s window writes
   0 without a DSM, and step 1 has turned that into -1 before step 3 looks.
   The ds flags are likewise read only where they were written: k_decomp
   skips signatures k_prep decided, and those are exactly step 1's. */
FD_DEV int
strict_decide( u32 i, u8 const * __restrict__ pub, u8 const * __restrict__ sig, int code, u8 const * __restrict__ ws,
               ws_layout_t L, int kind ) {
  /* R || s and A as LE dwords */
  uint4 const * S4 = (uint4 const *)(sig + 64UL*i);
  uint4 const * P4 = (uint4 const *)(pub + 32UL*i);
  uint4 const r0 = S4[0], r1 = S4[1], s0 = S4[2], s1 = S4[3], a0 = P4[0], a1 = P4[1];
  u32 const sw[8] = { s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w };
  u32 const Lw[8] = { 0x5cf5d3edu, 0x5812631au, 0xa2f79cd6u, 0x14def9deu, 0u, 0u, 0u, 0x10000000u };
  if( ge256( sw, Lw ) ) return -1;                                                   /* step 1 */
  if( code == -2 || strict_bad_encoding( a0, a1 ) || strict_bad_encoding( r0, r1 ) ||
      (ws[L.ds + 2u*i] | ws[L.ds + 2u*i + 1u]) ) return -2;                          /* step 2 */
  if( code == 0 || code == -3 ) {                                                    /* steps 3, 4 */
    size_t const N = L.N;
    i32 const * Ail = (i32 const *)(ws + L.Ai) + (size_t)i*384u;
    fe X, Y, Z;
    switch( kind ) {   /* a kernel argument or a chunk's mode: a scalar branch */
    case STRICT_DSM:  dsm_load_parked ( X, Y, Z, Ail ); break;
    case STRICT_DSM4: dsm4_load_parked( X, Y, Z, Ail ); break;
    case STRICT_DSM8: dsm8_load_parked( X, Y, Z, Ail ); break;
    default:          pool_load_parked( X, Y, Z, Ail, ((int const *)(ws + L.top))[i] ); break;
    }
    i32 const * Rw = (i32 const *)(ws + L.R);
    fe RX, RY;
    _Pragma("unroll") for( int k=0; k<10; k++ ) { RX.v[k] = Rw[(size_t)k*N + i]; RY.v[k] = Rw[(size_t)(10+k)*N + i]; }
    code = strict_point_eq( X, Y, Z, RX, RY ) ? 0 : -3;
  }
  return code;
}

/* One lane per signature.  err holds the reference pipeline's verdicts and
   receives the strict ones; out (NULL = none; the latency path's mapped
   host buffer) receives every final verdict, so that in strict mode no
   reference verdict reaches the host (k_dsm8 / k_dsm4 are then launched
   with out = NULL).  Untouched: slots with skip[i] != 0 (transaction slots
   that failed to parse) and slots carrying FD_AMD_VERDICT_DEVICE (k_dsmp's
   step guard tripped: k_fin marked the whole launch). */
__global__ void __launch_bounds__(64)
k_strict( u32 n, u8 const * __restrict__ pub, u8 const * __restrict__ sig, i8 * __restrict__ err,
          u8 const * __restrict__ ws, ws_layout_t L, i8 const * __restrict__ skip, int kind, i8 * __restrict__ out ) {
  u32 const i = blockIdx.x * 64u + threadIdx.x;
  if( i >= n ) return;
  int code = (int)err[i];
  if( !(skip && skip[i]) && code != FD_AMD_VERDICT_DEVICE ) {
    code = strict_decide( i, pub, sig, code, ws, L, kind );
    err[i] = (i8)code;
  }
  if( out ) out[i] = (i8)code;
}

#endif /* FD_ED25519_STRICT_H */
