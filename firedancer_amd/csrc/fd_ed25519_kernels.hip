/* firedancer_amd/csrc/fd_ed25519_kernels.hip
 *
 * The ed25519 verify pipeline as three CDNA4 kernels, one signature per
 * lane (64 signatures per wave64):
 *
 *   k_prep   s-range check (fd_ed25519_user.c:362-393), SHA-512(R||A||M)
 *            (user.c:411-413), reduction mod L (user.c:414), signed
 *            sliding-window recoding of h and s (avx/fd_ed25519_ge.c:378-400)
 *            -> digit planes in HBM.
 *   k_decomp 2-point decompression (avx/fd_ed25519_ge.c:221-299), one lane
 *            per point (A and R of a signature on adjacent lanes), then the
 *            A := -A negation (user.c:406-407).
 *   k_dsm    [h](-A) + [s]B with the reference's AVX op flow
 *            (avx/fd_ed25519_ge.c:408-527) run as a per-lane op stream (no
 *            predicated adds; the Ai table in a per-lane HBM slab, the Bi
 *            table in LDS) and the limb compare (user.c:417-425).
 *
 * Verdict per signature: err[i] in {0,-1,-2,-3}; 1 marks "still pending"
 * between kernels.
 *
 * The stages live in headers of this one translation unit, included below
 * in the order their kernels are laid out in the code object:
 *   fd_ed25519_ws.h     workspace layout
 *   fd_ed25519_front.h  k_prep, k_decomp, k_front
 *   fd_ed25519_dsm.h    group ops, step stream, k_dsm (1 lane per signature)
 *   fd_ed25519_dsm4.h   k_dsm4 (4 lanes)
 *   fd_ed25519_dsm8.h   k_dsm8 (8 lanes)
 *   fd_ed25519_pool.h   k_ai, k_dsmp, k_fin (large batches)
 *   fd_ed25519_tile.h   k_tile_persist, k_tile_synth
 *   fd_ed25519_strict.h k_strict (strict mode's overlay, after the DSM stage)
 *   fd_ed25519_gather.h k_gather, k_gather_txn (pointer-array chunks from registered memory)
 *   fd_ed25519_frags.h  k_frag_list, k_frag_check, k_frag_verdict (a submission's frags listed from the mcache lines)
 *   fd_ed25519_keep.h   k_keep_clear, k_keep_insert, k_keep_mark, k_keep_store (a batch's survivors)
 *   fd_ed25519_window.h k_win_clear, k_win_rebuild, k_win_query, k_win_insert, k_win_head (dedup across submissions)
 * This file keeps the launch code, the batch-size policy and the small
 * kernels that move results out (k_copy_out: verdicts; k_tag_out /
 * k_tag_gather: the dedup tags k_prep left in the workspace).
 */

#include "fd_ed25519_dev.h"
#include "fd_ed25519_kernels.h"
#include "fd_txn_dev.h"
#include <stdlib.h>

#include "fd_ed25519_ws.h"
#include "fd_ed25519_front.h"
#include "fd_ed25519_dsm.h"
#include "fd_ed25519_dsm4.h"
#include "fd_ed25519_dsm8.h"
#include "fd_ed25519_pool.h"
#include "fd_ed25519_tile.h"
#include "fd_ed25519_strict.h"
#include "../../include/fd_txn_amd.h"   /* FD_TXN_AMD_MTU: k_gather_txn's one pass */
#include "fd_ed25519_gather.h"
#include "fd_ed25519_frags.h"
#include "fd_ed25519_keep.h"
#include "fd_ed25519_window.h"
#include "fd_ed25519_emit.h"

/* ------------------------------------------------------------------ */
/* launch                                                               */

/* debug: dense u16 [n][256] digits from the event lists */
__global__ void __launch_bounds__(64)
k_digits_dense( u32 n, u8 const * __restrict__ ws, ws_layout_t L, u16 * __restrict__ out ) {
  u32 i = blockIdx.x * 64u + threadIdx.x;
  if( i >= n ) return;
  u16 * o = out + (size_t)i*256u;
  for( int k=0; k<256; k++ ) o[k] = 0;
  u32 ne = ((u32 const *)(ws + L.evn))[i];
  u16 const * ev = (u16 const *)(ws + L.dig) + (size_t)i*128u;
  for( u32 j=0; j<(ne & 0xffu); j++ )        { u16 e = ev[j];      o[e & 0xffu] = (u16)(o[e & 0xffu] | (e >> 8)); }
  for( u32 j=0; j<((ne >> 8) & 0xffu); j++ ) { u16 e = ev[64u + j]; o[e & 0xffu] = (u16)(o[e & 0xffu] | (e & 0xff00u)); }
}

int
fd_amd_launch_digits_dense( uint32_t n, void const * d_ws, uint16_t * d_dig, hipStream_t stream ) {
  if( !n ) return 0;
  hipLaunchKernelGGL( k_digits_dense, dim3((n + 63u)/64u), dim3(64), 0, stream, n, (u8 const *)d_ws, fd_amd_ws_layout( n ), d_dig );
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

/* Registered-memory batches: message offsets arrive as the caller wrote
   them (into its whole blob); the chunk's message window [lo, ...) was
   copied to the start of the device blob, so rebase them (empty messages
   point at 0, never outside the window). */
__global__ void __launch_bounds__(256)
k_rebase_off( u32 n, u32 * __restrict__ off, u32 const * __restrict__ sz, u32 lo ) {
  u32 i = blockIdx.x * 256u + threadIdx.x;
  if( i < n ) off[i] = sz[i] ? off[i] - lo : 0u;
}

int
fd_amd_launch_rebase_off( uint32_t n, uint32_t * d_off, uint32_t const * d_sz, uint32_t lo, hipStream_t stream ) {
  if( !n ) return 0;
  hipLaunchKernelGGL( k_rebase_off, dim3((n + 255u)/256u), dim3(256), 0, stream, n, d_off, d_sz, lo );
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

/* 4 GATHER_G records per wave and pass, at most `waves` waves (0: no cap) (k_gather, fd_ed25519_gather.h). */
int
fd_amd_launch_gather( uint32_t n, fd_amd_gather_rec_t const * d_rec, uint8_t * d_pub, uint8_t * d_sig, uint32_t * d_off,
                      uint32_t * d_sz, uint8_t * d_blob, uint32_t waves, hipStream_t stream ) {
  if( !n ) return 0;
  u32 const per = 4u*GATHER_G;
  u32 nb = (n + per - 1u)/per;
  if( waves && nb > waves ) nb = waves;
  hipLaunchKernelGGL( k_gather, dim3(nb), dim3(64), 0, stream, n, d_rec, d_pub, d_sig, d_off, d_sz, d_blob );
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

/* 4 GATHER_G payloads per wave, at most `waves` waves (0: no cap) (k_gather_txn, fd_ed25519_gather.h). */
int
fd_amd_launch_gather_txn( uint32_t n, fd_amd_gather_txn_rec_t const * d_rec, uint8_t * d_blob, uint32_t * d_toff,
                          uint32_t * d_tsz, uint32_t * d_tbase, uint32_t slot_cnt, uint32_t waves, hipStream_t stream ) {
  if( !n ) return 0;
  u32 const per = 4u*GATHER_G;
  u32 nb = (n + per - 1u)/per;
  if( waves && nb > waves ) nb = waves;
  hipLaunchKernelGGL( k_gather_txn, dim3(nb), dim3(64), 0, stream, n, d_rec, d_blob, d_toff, d_tsz, d_tbase, slot_cnt );
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

/* One lane per line / item (k_frag_list, k_frag_check, k_frag_verdict, fd_ed25519_frags.h). */
int
fd_amd_launch_frag_list( uint32_t n, void const * d_mcache, uint64_t depth, uint64_t seq0, uint64_t d_chunk0, uint64_t data_sz,
                         uint32_t frag_max, uint64_t d_idle, fd_amd_gather_rec_t * d_rec, int8_t * d_status, hipStream_t stream ) {
  if( !n ) return 0;
  u32 const stride = ( frag_max - FRAG_HDR + 15u ) & ~15u;
  hipLaunchKernelGGL( k_frag_list, dim3((n + 63u)/64u), dim3(64), 0, stream, n, (u8 const *)d_mcache, depth - 1UL, seq0, d_chunk0,
                      data_sz, frag_max, stride, d_idle, d_rec, d_status );
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int
fd_amd_launch_frag_check( uint32_t n, void const * d_mcache, uint64_t depth, uint64_t seq0, int8_t * d_status, hipStream_t stream ) {
  if( !n ) return 0;
  hipLaunchKernelGGL( k_frag_check, dim3((n + 63u)/64u), dim3(64), 0, stream, n, (u8 const *)d_mcache, depth - 1UL, seq0, d_status );
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int
fd_amd_launch_frag_verdict( uint32_t n, int8_t * d_status, void const * d_mcache, uint64_t depth, uint64_t seq0, int8_t * d_err,
                            int8_t * m_err, void * d_ws, hipStream_t stream ) {
  if( !n ) return 0;
  hipLaunchKernelGGL( k_frag_verdict, dim3((n + 63u)/64u), dim3(64), 0, stream, n, d_status, (u8 const *)d_mcache, depth - 1UL, seq0,
                      d_err, m_err, (u64 *)((u8 *)d_ws + fd_amd_ws_layout( n ).tag) );
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

/* device -> mapped host result copy: 16 B per lane where both ends are
   16-aligned (every result buffer is), bytes otherwise. */
__global__ void __launch_bounds__(256)
k_copy_out( u8 * __restrict__ dst, u8 const * __restrict__ src, size_t n ) {
  size_t i = (size_t)blockIdx.x * 256u + threadIdx.x, stride = (size_t)gridDim.x * 256u;
  size_t nv = (((size_t)dst | (size_t)src) & 15u) ? 0 : (n >> 4);
  for( size_t k = i; k < nv; k += stride ) ((uint4 *)dst)[k] = ((uint4 const *)src)[k];
  for( size_t k = (nv << 4) + i; k < n; k += stride ) dst[k] = src[k];
}

int
fd_amd_launch_copy_out( void * d_dst, void const * d_src, size_t n, hipStream_t stream ) {
  if( !n ) return 0;
  size_t nb = ( (n >> 4) + 256u ) / 256u;
  if( nb > 4096u ) nb = 4096u;
  hipLaunchKernelGGL( k_copy_out, dim3((unsigned)nb), dim3(256), 0, stream, (u8 *)d_dst, (u8 const *)d_src, n );
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

/* Dedup tags: the tag plane k_prep / k_front left in the workspace -> dst,
   device or mapped host memory.  16 B (two tags) per lane where dst is
   16-aligned (the plane is 256-aligned), one tag per lane otherwise. */
__global__ void __launch_bounds__(256)
k_tag_out( u64 * __restrict__ dst, u64 const * __restrict__ tag, size_t n ) {
  size_t i = (size_t)blockIdx.x * 256u + threadIdx.x, stride = (size_t)gridDim.x * 256u;
  size_t nv = ((size_t)dst & 15u) ? 0 : (n >> 1);
  for( size_t k = i; k < nv; k += stride ) ((ulong2 *)dst)[k] = ((ulong2 const *)tag)[k];
  for( size_t k = (nv << 1) + i; k < n; k += stride ) dst[k] = tag[k];
}

/* The gather form: dst[t] = the tag of transaction t's first signature slot,
   tag[tbase[t]]; 0 for a transaction without a slot.  A payload that failed
   to parse either reserved no slot or had every slot skipped, and k_prep
   writes tag 0 for a skipped slot; a payload that parsed has at least one
   signature (fd_txn_parse.c:81).  The plane's offset depends on the slot
   count the verify was launched with, tbase[txn_cnt]. */
__global__ void __launch_bounds__(256)
k_tag_gather( u64 * __restrict__ dst, u8 const * __restrict__ ws, u32 txn_cnt, u32 const * __restrict__ tbase ) {
  u32 t = blockIdx.x * 256u + threadIdx.x;
  if( t >= txn_cnt ) return;
  u32 slots = tbase[txn_cnt], b = tbase[t], e = tbase[t+1u];
  u64 const * tag = (u64 const *)(ws + ws_layout_const( slots ).tag);
  dst[t] = ( b < e && b < slots ) ? tag[b] : 0UL;
}

int
fd_amd_launch_tag_out( void * d_dst, void const * d_ws, size_t n, hipStream_t stream ) {
  if( !n ) return 0;
  size_t nb = ( (n >> 1) + 256u ) / 256u;
  if( nb > 4096u ) nb = 4096u;
  hipLaunchKernelGGL( k_tag_out, dim3((unsigned)nb), dim3(256), 0, stream, (u64 *)d_dst,
                      (u64 const *)((u8 const *)d_ws + fd_amd_ws_layout( n ).tag), n );
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int
fd_amd_launch_tag_gather( void * d_dst, void const * d_ws, uint32_t txn_cnt, uint32_t const * d_tbase, hipStream_t stream ) {
  if( !txn_cnt ) return 0;
  hipLaunchKernelGGL( k_tag_gather, dim3((txn_cnt + 255u)/256u), dim3(256), 0, stream, (u64 *)d_dst, (u8 const *)d_ws,
                      txn_cnt, d_tbase );
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

/* Kernel choice by batch size: up to g_dsm8_max signatures k_dsm8 (8 lanes
   per signature: the shortest op stream, but twice k_dsm4's waves), up to
   g_dsm4_max k_dsm4, larger batches k_dsm.  Measured (profiles/
   r02_k_dsm4_latency_experiments.txt): k_dsm8 is faster while its waves fit
   one per SIMD (n <= 8192 on 1024 SIMDs), slower beyond. */
static volatile u32 g_dsm4_max = 16384u;
static volatile u32 g_dsm8_max = 8192u;
static volatile u32 g_pool_min = 1u << 19;   /* k_dsmp from 2^19 signatures (pooled A/B) */
static volatile u64 g_pool_iter_cap = ~0UL;   /* debug: cap on k_dsmp's step loop (its hang guard) */
static volatile u32 g_pool_waves_dbg = 0u;    /* debug: k_dsmp's grid whatever the batch size (0: the policy) */

extern "C" void
fd_ed25519_amd_debug_set_pool_iter_cap( unsigned long cap ) {
  g_pool_iter_cap = cap ? cap : ~0UL;
}

extern "C" void
fd_ed25519_amd_debug_set_pool_waves( unsigned long w ) {
  g_pool_waves_dbg = w > 0xFFFFFFFFUL ? 0xFFFFFFFFu : (u32)w;
}

extern "C" void
fd_ed25519_amd_set_pool_batch_min( unsigned long n ) {
  g_pool_min = n > 0xFFFFFFFFUL ? 0xFFFFFFFFu : (u32)n;
}

/* k_dsmp grid: one single-wave workgroup per resident wave slot (8 per CU:
   LDS-bound at FD_POOL_P slots, VGPR-bound at 2 waves per SIMD), fewer
   when the batch would leave pools nearly empty.  The debug override
   (fd_ed25519_amd_debug_set_pool_waves) replaces only the batch-size term:
   tests use it to make few waves refill their slots at a small n. */
static u32
pool_waves( u32 n ) {
  static int cus = 0;
  if( !cus ) {
    int dev = 0, v = 0;
    if( hipGetDevice( &dev ) != hipSuccess || hipDeviceGetAttribute( &v, hipDeviceAttributeMultiprocessorCount, dev ) != hipSuccess || v <= 0 ) v = 256;
    cus = v;
  }
  u32 wmax = 8u * (u32)cus;
#ifdef FD_AMD_DIAG
  if( char const * e = getenv( "FD_POOL_WAVES" ) ) { u32 v = (u32)atoi( e ); if( v ) wmax = v; }
#endif
  u32 const dbg = g_pool_waves_dbg;
  if( dbg ) return dbg < wmax ? dbg : wmax;
  u32 want = (n + 63u) / 64u;
  return want < wmax ? (want ? want : 1u) : wmax;
}

extern "C" void
fd_ed25519_amd_set_small_batch_max( unsigned long n ) {
  g_dsm4_max = n > 0xFFFFFFFFUL ? 0xFFFFFFFFu : (u32)n;
}

extern "C" void
fd_ed25519_amd_set_latency_batch_max( unsigned long n ) {
  g_dsm8_max = n > 0xFFFFFFFFUL ? 0xFFFFFFFFu : (u32)n;
}

int
fd_amd_uses_latency_path( uint32_t n, int dsm_mode ) {
  return dsm_mode == 2 || dsm_mode == 3 || (dsm_mode == 0 && (n <= g_dsm4_max || n <= g_dsm8_max));
}

/* The DSM kernel a batch of n runs: the one place that applies the size
   rule, for the launch below and for the R' read-back (which must decode the
   parking layout of the kernel the launch chose). */
int
fd_amd_dsm_kind( uint32_t n, int dsm_mode ) {
  if( fd_amd_uses_latency_path( n, dsm_mode ) )
    return ( dsm_mode == 3 || (dsm_mode == 0 && n <= g_dsm8_max) ) ? STRICT_DSM8 : STRICT_DSM4;
  return ( dsm_mode == 4 || (dsm_mode == 0 && n >= g_pool_min) ) ? STRICT_DSMP : STRICT_DSM;
}

/* debug: the R' = (X, Y, Z) each signature's DSM parked in its Ai slab, read
   through the parking layout of DSM kernel `kind` (k_strict's own loaders)
   -> int32 [30][n], X | Y | Z limbs.  Rows of signatures whose DSM did not
   run are whatever the slab holds. */
__global__ void __launch_bounds__(64)
k_rprime( u32 n, u8 const * __restrict__ ws, ws_layout_t L, int kind, i32 * __restrict__ out ) {
  u32 const i = blockIdx.x * 64u + threadIdx.x;
  if( i >= n ) return;
  i32 const * Ail = (i32 const *)(ws + L.Ai) + (size_t)i*384u;
  fe X, Y, Z;
  switch( kind ) {
  case STRICT_DSM:  dsm_load_parked ( X, Y, Z, Ail ); break;
  case STRICT_DSM4: dsm4_load_parked( X, Y, Z, Ail ); break;
  case STRICT_DSM8: dsm8_load_parked( X, Y, Z, Ail ); break;
  default:          pool_load_parked( X, Y, Z, Ail, ((int const *)(ws + L.top))[i] ); break;
  }
  _Pragma("unroll") for( int k=0; k<10; k++ ) {
    out[(size_t)k*n + i] = X.v[k]; out[(size_t)(10+k)*n + i] = Y.v[k]; out[(size_t)(20+k)*n + i] = Z.v[k];
  }
}

int
fd_amd_launch_rprime( uint32_t n, void const * d_ws, int kind, int32_t * d_xyz, hipStream_t stream ) {
  if( !n ) return 0;
  if( !kind ) kind = fd_amd_dsm_kind( n, 0 );
  if( kind < STRICT_DSM || kind > STRICT_DSMP ) return -1;
  hipLaunchKernelGGL( k_rprime, dim3((n + 63u)/64u), dim3(64), 0, stream, n, (u8 const *)d_ws, fd_amd_ws_layout( n ), kind, d_xyz );
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int
fd_amd_launch_verify( u32 n, u8 const * d_pub, u8 const * d_sig, u32 const * d_off, u32 const * d_sz,
                      u8 const * d_blob, i8 * d_err, void * d_ws, hipStream_t stream, int want_stats,
                      hipEvent_t const * ev, i8 const * d_skip, int dsm_mode, i8 * d_out, int strict ) {
  if( !n ) return 0;
  ws_layout_t L = fd_amd_ws_layout( n );
  u8 * ws = (u8 *)d_ws;
  u32 nb = (n + 63u) / 64u;
  int const kind = fd_amd_dsm_kind( n, dsm_mode );
  bool const small = kind == STRICT_DSM4 || kind == STRICT_DSM8, eight = kind == STRICT_DSM8, pooled = kind == STRICT_DSMP;
  /* strict mode: k_strict writes the verdicts that go to d_out, the DSM kernel none */
  i8 * const dsm_out = strict ? NULL : d_out;
  if( ev ) (void)hipEventRecord( ev[0], stream );
  if( small ) {   /* latency path: one front launch (hash || decompress), then k_dsm8 or k_dsm4 */
    hipLaunchKernelGGL( k_front, dim3(3u*nb), dim3(64), 0, stream, n, nb, d_pub, d_sig, d_off, d_sz, d_blob, d_err, ws, L, d_skip );
    if( ev ) { (void)hipEventRecord( ev[1], stream ); (void)hipEventRecord( ev[2], stream ); }
    if( eight ) hipLaunchKernelGGL( k_dsm8, dim3((n + 7u)/8u), dim3(64), 0, stream, n, d_err, ws, L, want_stats, dsm_out );
    else        hipLaunchKernelGGL( k_dsm4, dim3((n + 15u)/16u), dim3(64), 0, stream, n, d_err, ws, L, want_stats, dsm_out );
  } else {
    hipLaunchKernelGGL( k_prep,   dim3(nb),    dim3(64), 0, stream, n, d_pub, d_sig, d_off, d_sz, d_blob, d_err, ws, L, d_skip );
    if( ev ) (void)hipEventRecord( ev[1], stream );
    hipLaunchKernelGGL( k_decomp, dim3(2u*nb), dim3(64), 0, stream, n, d_pub, d_sig, d_err, ws, L );
    if( ev ) (void)hipEventRecord( ev[2], stream );
    if( pooled ) {
      hipLaunchKernelGGL( k_ai,   dim3(nb),    dim3(64), 0, stream, n, d_err, ws, L );
      hipLaunchKernelGGL( k_dsmp, dim3(pool_waves( n )), dim3(64), 0, stream, n, ws, L, (u64)g_pool_iter_cap );
      hipLaunchKernelGGL( k_fin,  dim3(nb),    dim3(64), 0, stream, n, d_err, ws, L, want_stats );
    } else {
      hipLaunchKernelGGL( k_dsm,  dim3(nb),    dim3(64), 0, stream, n, d_err, ws, L, want_stats );
    }
  }
  if( strict )   /* the overlay: re-decide every verdict (fd_ed25519_strict.h); d_out as the DSM kernel would have used it */
    hipLaunchKernelGGL( k_strict, dim3(nb), dim3(64), 0, stream, n, d_pub, d_sig, d_err, (u8 const *)ws, L, d_skip, kind,
                        small ? d_out : (i8 *)NULL );
  if( ev ) (void)hipEventRecord( ev[3], stream );
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
