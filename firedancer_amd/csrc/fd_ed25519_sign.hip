/* firedancer_amd/csrc/fd_ed25519_sign.hip
 *
 * GPU keygen + sign: synthesises large verify workloads
 * (2^24 signatures for config 4) on the device instead of host threads.
 * Ed25519 signing is deterministic (RFC 8032 s5.1.6), so the output bytes
 * equal the reference's fd_ed25519_public_from_private / fd_ed25519_sign
 * (src/ballet/ed25519/fd_ed25519_user.c:279-343) for any correct
 * algorithm; tests compare every byte with an independent big-integer
 * model of RFC 8032 and with the host signer, and probe each device
 * function of fd_ed25519_sign.h alone.  One signature per lane:
 *
 *   h = SHA-512(seed); a = clamp(h[0:32]); A = [a]B   -> public key
 *   r = SHA-512(h[32:64] || M) mod L; R = [r]B
 *   k = SHA-512(R || A || M) mod L;  S = (r + k a) mod L  -> R || S
 *
 * [x]B is the signed radix-16 fixed-base method over the 32 x 8 table
 * BASE[j][k] = (k+1) 256^j B (tools/gen_consts.py): 64 mixed additions and
 * 4 doublings; points are encoded with one inversion each.  Not constant
 * time: workload synthesis only, never for real keys.
 */
#include "fd_ed25519_sign.h"
#include "fd_ed25519_kernels.h"

__global__ void __launch_bounds__(64)
k_sign( u32 n, u8 const * __restrict__ prv, u32 const * __restrict__ moff, u32 const * __restrict__ msz,
        u8 const * __restrict__ blob, u8 * __restrict__ pub, u8 * __restrict__ sig ) {
  u32 i = blockIdx.x * 64u + threadIdx.x;
  if( i >= n ) return;
  u32 const * P = (u32 const *)(prv + 32UL*i);                      /* 32-aligned records */
  u64 seed[4];
  _Pragma("unroll") for( int k=0; k<4; k++ ) seed[k] = ((u64)P[2*k+1] << 32) | P[2*k];
  u64 st[8];
  sha512_pm<4>( st, seed, (u8 const *)0, 0u );
  u32 hw[16]; digest_words( hw, st );
  u32 a[8];
  _Pragma("unroll") for( int k=0; k<8; k++ ) a[k] = hw[k];
  a[0] &= ~7u; a[7] &= 0x7fffffffu; a[7] |= 0x40000000u;          /* clamp (RFC 8032 s5.1.5) */
  u32 A[8]; scalarmult_base_enc( A, a );
  u32 * PO = (u32 *)(pub + 32UL*i);
  _Pragma("unroll") for( int k=0; k<8; k++ ) PO[k] = A[k];

  u8 const * M = blob + moff[i];
  u32 sz = msz[i];
  u64 pre[4];
  _Pragma("unroll") for( int k=0; k<4; k++ ) pre[k] = ((u64)hw[8+2*k+1] << 32) | hw[8+2*k];
  sha512_pm<4>( st, pre, M, sz );
  u32 rw[16]; digest_words( rw, st );
  u32 r[8]; sc_reduce( r, rw );
  u32 R[8]; scalarmult_base_enc( R, r );

  u64 ra[8];
  _Pragma("unroll") for( int k=0; k<4; k++ ) { ra[k] = ((u64)R[2*k+1] << 32) | R[2*k]; ra[4+k] = ((u64)A[2*k+1] << 32) | A[2*k]; }
  sha512_pm<8>( st, ra, M, sz );
  u32 kw[16]; digest_words( kw, st );
  u32 kk[8]; sc_reduce( kk, kw );
  /* a itself may exceed L: reduce it first (ka mod L is unchanged) */
  u32 aw[16];
  _Pragma("unroll") for( int k=0; k<8; k++ ) { aw[k] = a[k]; aw[8+k] = 0u; }
  u32 ar[8]; sc_reduce( ar, aw );
  u32 S[8]; sc_muladd( S, kk, ar, r );
  u32 * SO = (u32 *)(sig + 64UL*i);
  _Pragma("unroll") for( int k=0; k<8; k++ ) { SO[k] = R[k]; SO[8+k] = S[k]; }
}

int
fd_amd_launch_sign( uint32_t n, uint8_t const * d_prv, uint32_t const * d_off, uint32_t const * d_sz,
                    uint8_t const * d_blob, uint8_t * d_pub, uint8_t * d_sig, hipStream_t stream ) {
  if( !n ) return 0;
  hipLaunchKernelGGL( k_sign, dim3((n + 63u)/64u), dim3(64), 0, stream, n, d_prv, d_off, d_sz, d_blob, d_pub, d_sig );
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
