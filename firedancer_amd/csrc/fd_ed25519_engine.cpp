/* firedancer_amd/csrc/fd_ed25519_engine.cpp
 *
 * Host side of the C-ABI boundary (include/fd_ed25519_amd.h): the batch
 * engine (device buffers, pinned double-buffered staging, per-engine HIP
 * streams), the device-resident entry point, and the reference's drop-in
 * fd_ed25519_verify / fd_ed25519_strerror.
 *
 * Reference interfaces replaced: src/ballet/ed25519/fd_ed25519.h:96-109
 * (verify, strerror); the tile-side call site is
 * src/app/frank/load/fd_frank_verify_synth_load.c:380 (one verify per
 * fragment); the batch API is new (SURVEY.md s8 b).
 */
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <vector>
#include <pthread.h>
#include <sys/random.h>
#include <sys/syscall.h>
#include <time.h>
#include <unistd.h>
#include <thread>

#include "../../include/fd_ed25519_amd.h"
#include "../../include/fd_txn_amd.h"
#include "../../include/fd_tango_amd.h"   /* frag submissions */
#include "fd_ed25519_kernels.h"
#include "fd_ed25519_emit.h"   /* the layout arithmetic alone: no kernel is compiled here */
#include "fd_txn_budget.h"     /* likewise: the record's codes, for the asserts below */

#define HIPCHK( x ) do { hipError_t _e = (x); if( _e != hipSuccess ) {                          \
    fprintf( stderr, "fd_ed25519_amd: %s failed: %s (%s:%d)\n", #x, hipGetErrorString( _e ),     \
             __FILE__, __LINE__ );                                                              \
    return FD_ED25519_AMD_ERR_DEVICE; } } while(0)

#include "fd_ed25519_engine.h"

/* Results go device -> host through a small kernel that writes the mapped,
   coherent pinned buffer, not through a DMA copy: the copy engine serves
   the streams' commands in order, so a D2H queued behind one batch's
   kernels would hold up the next batch's H2D on another stream. */
static hipError_t
slot_out( slot_t * s, void * m_dst /* s->m_err or s->m_terr */, void const * d_src, ulong n ) {
  return fd_amd_launch_copy_out( m_dst, d_src, n, s->stream ) ? hipErrorLaunchFailure : hipSuccess;
}

static void
slot_free( slot_t * s ) {
  if( s->d_pub  ) (void)hipFree( s->d_pub );
  if( s->d_sig  ) (void)hipFree( s->d_sig );
  if( s->d_blob ) (void)hipFree( s->d_blob );
  if( s->d_off  ) (void)hipFree( s->d_off );
  if( s->d_sz   ) (void)hipFree( s->d_sz );
  if( s->d_err  ) (void)hipFree( s->d_err );
  if( s->d_ws   ) (void)hipFree( s->d_ws );
  if( s->h_blob ) (void)hipHostFree( s->h_blob );
  if( s->h_err  ) (void)hipHostFree( s->h_err );
  if( s->d_pack ) (void)hipFree( s->d_pack );
  if( s->h_pack ) (void)hipHostFree( s->h_pack );
  if( s->d_toff ) (void)hipFree( s->d_toff );
  if( s->d_tsz  ) (void)hipFree( s->d_tsz );
  if( s->d_fp   ) (void)hipFree( s->d_fp );
  if( s->d_tbase) (void)hipFree( s->d_tbase );
  if( s->d_terr ) (void)hipFree( s->d_terr );
  if( s->d_skip ) (void)hipFree( s->d_skip );
  if( s->h_toff ) (void)hipHostFree( s->h_toff );
  if( s->h_tsz  ) (void)hipHostFree( s->h_tsz );
  if( s->h_tbase) (void)hipHostFree( s->h_tbase );
  if( s->h_terr ) (void)hipHostFree( s->h_terr );
  if( s->h_tag  ) (void)hipHostFree( s->h_tag );
  if( s->d_dpack) (void)hipFree( s->d_dpack );
  if( s->h_dpack) (void)hipHostFree( s->h_dpack );
  if( s->d_kpack) (void)hipFree( s->d_kpack );
  if( s->h_kpack) (void)hipHostFree( s->h_kpack );
  if( s->d_epack) (void)hipFree( s->d_epack );
  if( s->h_epack) (void)hipHostFree( s->h_epack );
  if( s->h_budget) (void)hipHostFree( s->h_budget );
  if( s->d_fpack ) (void)hipFree( s->d_fpack );
  if( s->win_done ) (void)hipEventDestroy( s->win_done );
  if( s->stream ) (void)hipStreamDestroy( s->stream );
  if( s->done   ) (void)hipEventDestroy( s->done );
  memset( s, 0, sizeof(*s) );
}

static int
slot_alloc( slot_t * s, ulong cap, ulong blob_cap ) {
  memset( s, 0, sizeof(*s) );
  ws_layout_t L = fd_amd_ws_layout( cap );
  HIPCHK( hipMalloc( (void **)&s->d_pub,  32UL*cap ) );
  HIPCHK( hipMalloc( (void **)&s->d_sig,  64UL*cap ) );
  HIPCHK( hipMalloc( (void **)&s->d_blob, blob_cap + 64UL ) );
  HIPCHK( hipMalloc( (void **)&s->d_off,  4UL*cap ) );
  HIPCHK( hipMalloc( (void **)&s->d_sz,   4UL*cap ) );
  HIPCHK( hipMalloc( (void **)&s->d_err,  cap ) );
  HIPCHK( hipMalloc( &s->d_ws, L.total ) );
  HIPCHK( hipHostMalloc( (void **)&s->h_blob, blob_cap + 64UL, hipHostMallocDefault ) );
  HIPCHK( hipHostMalloc( (void **)&s->h_err,  cap, hipHostMallocMapped | hipHostMallocCoherent ) );
  HIPCHK( hipHostGetDevicePointer( &s->m_err, s->h_err, 0 ) );
  HIPCHK( hipMalloc( (void **)&s->d_pack, 104UL*cap + blob_cap + 64UL ) );
  HIPCHK( hipHostMalloc( (void **)&s->h_pack, 104UL*cap + blob_cap + 64UL, hipHostMallocMapped | hipHostMallocCoherent ) );
  HIPCHK( hipHostGetDevicePointer( (void **)&s->m_pack, s->h_pack, 0 ) );
  HIPCHK( hipStreamCreateWithFlags( &s->stream, hipStreamNonBlocking ) );
  HIPCHK( hipEventCreateWithFlags( &s->done, hipEventDisableTiming ) );
  /* first use of a stream (its hardware queue) and of a staging pair costs
     ~8 ms inside the first hipMemcpyAsync: pay it here, not in a batch */
  memset( s->h_pack, 0, 104UL*cap + blob_cap + 64UL );
  HIPCHK( hipMemcpyAsync( s->d_pack, s->h_pack, 104UL*cap + blob_cap + 64UL, hipMemcpyHostToDevice, s->stream ) );
  HIPCHK( hipStreamSynchronize( s->stream ) );
  return FD_ED25519_AMD_OK;
}

/* The slots' completion words (fd_ed25519_engine.h): mapped and coherent as
   h_err is, 64 bytes apart so that no two slots' stores share a line, zero
   to begin with (no ticket is 0). */
static int
engine_alloc_ticks( fd_ed25519_amd_t * e ) {
  HIPCHK( hipHostMalloc( (void **)&e->h_tickbuf, 64UL*(ulong)e->nslot, hipHostMallocMapped | hipHostMallocCoherent ) );
  memset( e->h_tickbuf, 0, 64UL*(ulong)e->nslot );
  void * m = NULL;
  HIPCHK( hipHostGetDevicePointer( &m, e->h_tickbuf, 0 ) );
  for( int k=0; k<e->nslot; k++ ) {
    e->slot[k].h_tick = (ulong *)(e->h_tickbuf + 64UL*(ulong)k);
    e->slot[k].m_tick = (uint8_t *)m + 64UL*(ulong)k;
  }
  return FD_ED25519_AMD_OK;
}

extern "C" fd_ed25519_amd_t *
fd_ed25519_amd_new( int device, ulong batch_max, ulong blob_max ) {
  ulong nslot = 2UL;
  char const * ev = getenv( "FD_ED25519_AMD_NSLOT" );
  if( ev && atoi( ev ) >= 2 && atoi( ev ) <= FD_AMD_SLOT_MAX ) nslot = (ulong)atoi( ev );
  return fd_ed25519_amd_new_slots( device, batch_max, blob_max, nslot );
}

extern "C" fd_ed25519_amd_t *
fd_ed25519_amd_new_slots( int device, ulong batch_max, ulong blob_max, ulong slots ) {
  if( slots < 2UL || slots > (ulong)FD_AMD_SLOT_MAX ) return NULL;   /* before anything touches a device */
  int const nslot = (int)slots;
  char const * ev;
  if( !batch_max ) batch_max = 1;
  if( batch_max > (1UL<<26) ) return NULL;
  if( blob_max < FD_ED25519_AMD_MSG_MAX ) blob_max = FD_ED25519_AMD_MSG_MAX;
  if( blob_max > (1UL<<32) - 4096UL ) return NULL;
  int cnt = 0;
  if( hipGetDeviceCount( &cnt ) != hipSuccess || device < 0 || device >= cnt ) {
    fprintf( stderr, "fd_ed25519_amd: no HIP device %d (count %d)\n", device, cnt );
    return NULL;
  }
  if( hipSetDevice( device ) != hipSuccess ) return NULL;
  fd_ed25519_amd_t * e = (fd_ed25519_amd_t *)calloc( 1, sizeof(fd_ed25519_amd_t) );
  if( !e ) return NULL;
  e->device = device; e->cap = batch_max; e->blob_cap = blob_max; e->nslot = nslot;
  ev = getenv( "FD_ED25519_AMD_GATHER_COPY" );
  e->gather_copy = ev && atoi( ev ) == 1;
  ev = getenv( "FD_ED25519_AMD_GATHER_TXN_WAVES" );
  e->gather_txn_waves = ( ev && atoi( ev ) >= 1 && atoi( ev ) <= 65536 ) ? atoi( ev ) : 64;
  /* the pinned staging on the GPU's NUMA node (the thread's own policy is
     restored afterwards; fd_numa.cpp) */
  int pmode = 0; unsigned long pmask[16];
  int pnode = fd_amd_numa_prefer_begin( device, &pmode, pmask );
  int bad = 0;
  for( int k=0; k<nslot && !bad; k++ ) bad = slot_alloc( &e->slot[k], batch_max, blob_max );
  if( !bad ) bad = engine_alloc_ticks( e );
  if( pnode >= 0 ) fd_amd_numa_prefer_end( pmode, pmask );
  if( bad ) { fd_ed25519_amd_delete( e ); return NULL; }
  ev = getenv( "FD_ED25519_AMD_ASYNC_POLL" );
  e->poll_event = ev && !strcmp( ev, "event" );
  /* the survivor filter's salt: a secret of this engine, from the OS; the
     clock only where that fails (slot_alloc cleared the slots: set it last) */
  if( getrandom( &e->salt, sizeof(e->salt), 0 ) != (ssize_t)sizeof(e->salt) ) {
    struct timespec ts; (void)clock_gettime( CLOCK_MONOTONIC, &ts );
    e->salt = ( (ulong)ts.tv_sec * 1000000007UL ) ^ ( (ulong)ts.tv_nsec << 21 ) ^ (ulong)(uintptr_t)e;
  }
  for( int k=0; k<nslot; k++ ) e->slot[k].salt = e->salt;
  return e;
}

extern "C" void
fd_ed25519_amd_delete( fd_ed25519_amd_t * e ) {
  if( !e ) return;
  (void)hipSetDevice( e->device );
  for( int k=0; k<FD_AMD_SLOT_MAX; k++ ) { if( e->slot[k].stream ) (void)hipStreamSynchronize( e->slot[k].stream ); slot_free( &e->slot[k] ); }
  if( e->win ) { e->win->pend = NULL; e->win->owner = NULL; }   /* the borrowed window: nothing of it is queued any more */
  if( e->h_tickbuf ) (void)hipHostFree( e->h_tickbuf );
  free( e );
}

/* The slot's transaction buffers, on its first transaction chunk. */
static int
slot_alloc_aux( slot_t * s, ulong cap ) {
  if( s->d_toff ) return FD_ED25519_AMD_OK;
  HIPCHK( hipMalloc( (void **)&s->d_toff,  4UL*cap ) );
  HIPCHK( hipMalloc( (void **)&s->d_tsz,   4UL*cap ) );
  HIPCHK( hipMalloc( (void **)&s->d_fp,    4UL*cap ) );
  HIPCHK( hipMalloc( (void **)&s->d_tbase, 4UL*(cap+1UL) ) );
  HIPCHK( hipMalloc( (void **)&s->d_terr,  cap ) );
  HIPCHK( hipMalloc( (void **)&s->d_skip,  cap ) );
  HIPCHK( hipHostMalloc( (void **)&s->h_toff,  4UL*cap, hipHostMallocDefault ) );
  HIPCHK( hipHostMalloc( (void **)&s->h_tsz,   4UL*cap, hipHostMallocDefault ) );
  HIPCHK( hipHostMalloc( (void **)&s->h_tbase, 4UL*(cap+1UL), hipHostMallocDefault ) );
  HIPCHK( hipHostMalloc( (void **)&s->h_terr,  cap, hipHostMallocMapped | hipHostMallocCoherent ) );
  HIPCHK( hipHostGetDevicePointer( &s->m_terr, s->h_terr, 0 ) );
  return FD_ED25519_AMD_OK;
}

/* The slot's tag buffers, on the first chunk whose caller asked for tags. */
static int
slot_alloc_tag( slot_t * s, ulong cap ) {
  if( s->h_tag ) return FD_ED25519_AMD_OK;
  HIPCHK( hipHostMalloc( (void **)&s->h_tag, 16UL*cap, hipHostMallocMapped | hipHostMallocCoherent ) );
  HIPCHK( hipHostGetDevicePointer( &s->m_tag, s->h_tag, 0 ) );
  s->h_ttag = s->h_tag + cap;
  s->m_ttag = (ulong *)s->m_tag + cap;
  return FD_ED25519_AMD_OK;
}

/* A chunk's worst case of packed descriptor bytes: every transaction at most
   FD_TXN_MAX_SZ (payloads are <= FD_TXN_AMD_MTU here), and by
   fd_txn_amd_desc_bound at most 20 + 10*sz/3 each with the sizes summing to
   at most blob_cap.  A multiple of 256. */
static ulong
desc_stage_sz( ulong cap, ulong blob_cap ) {
  ulong a = FD_TXN_MAX_SZ*cap, b = 20UL*cap + 10UL*blob_cap/3UL;
  return ( ( a < b ? a : b ) + 255UL ) & ~255UL;
}

/* The slot's descriptor staging, on the first chunk whose caller asked for
   descriptors. */
static int
slot_alloc_desc( slot_t * s, ulong cap, ulong blob_cap ) {
  if( s->d_dpack ) return FD_ED25519_AMD_OK;
  ulong const stage = desc_stage_sz( cap, blob_cap );
  ulong const off_sz = ( 8UL*(cap+1UL) + 255UL ) & ~255UL, bs_sz = ( 8UL*((cap+63UL)/64UL) + 255UL ) & ~255UL;
  HIPCHK( hipMalloc( (void **)&s->d_dpack, off_sz + bs_sz + stage ) );
  s->d_doff = (ulong *)s->d_dpack; s->d_dbsum = (ulong *)(s->d_dpack + off_sz); s->d_desc = s->d_dpack + off_sz + bs_sz;
  HIPCHK( hipHostMalloc( (void **)&s->h_dpack, off_sz + stage, hipHostMallocMapped | hipHostMallocCoherent ) );
  s->h_doff = (ulong *)s->h_dpack; s->h_desc = s->h_dpack + off_sz;
  HIPCHK( hipHostGetDevicePointer( &s->m_doff, s->h_dpack, 0 ) );
  s->m_desc = (uint8_t *)s->m_doff + off_sz;
  s->desc_stage = stage;
  return FD_ED25519_AMD_OK;
}

/* The slot's survivor buffers, on the first submission that asks for the
   publish list. */
static int
slot_alloc_keep( slot_t * s, ulong cap ) {
  if( s->d_kpack ) return FD_ED25519_AMD_OK;
  /* scr: a multiple of 256; the window's planes behind the filter's, used only with a window attached */
  ulong const scr = fd_amd_win_scratch( cap ).total, pl = ( 8UL*cap + 255UL ) & ~255UL;
  HIPCHK( hipEventCreateWithFlags( &s->win_done, hipEventDisableTiming ) );
  HIPCHK( hipMalloc( (void **)&s->d_kpack, scr + 2UL*pl ) );
  s->d_kscr = s->d_kpack; s->d_ktag = (ulong *)(s->d_kpack + scr); s->d_fpk = (uint32_t *)(s->d_kpack + scr + pl);
  HIPCHK( hipHostMalloc( (void **)&s->h_kpack, 256UL + 4UL*cap, hipHostMallocMapped | hipHostMallocCoherent ) );
  s->h_kcnt = (ulong *)s->h_kpack; s->h_keep = (uint *)(s->h_kpack + 256UL);
  HIPCHK( hipHostGetDevicePointer( &s->m_kcnt, s->h_kpack, 0 ) );
  s->m_keep = (uint8_t *)s->m_kcnt + 256UL;
  return FD_ED25519_AMD_OK;
}

/* The slot's output-frame buffers, on the first submission that asks for
   frames. */
static int
slot_alloc_emit( slot_t * s, ulong cap ) {
  if( s->d_epack ) return FD_ED25519_AMD_OK;
  ulong const off_sz = ( 8UL*(cap+1UL) + 255UL ) & ~255UL;
  HIPCHK( hipMalloc( (void **)&s->d_epack, fd_amd_emit_layout( cap ).total ) );
  HIPCHK( hipHostMalloc( (void **)&s->h_epack, off_sz + 4UL*cap, hipHostMallocMapped | hipHostMallocCoherent ) );
  s->h_eoff = (ulong *)s->h_epack; s->h_esz = (uint *)(s->h_epack + off_sz);
  HIPCHK( hipHostGetDevicePointer( &s->m_eoff, s->h_epack, 0 ) );
  s->m_esz = (uint8_t *)s->m_eoff + off_sz;
  return FD_ED25519_AMD_OK;
}

/* The slot's budget plane, on the first chunk whose caller asked for the
   compute budget: batch_max records that k_txn_budget writes in place. */
static int
slot_alloc_budget( slot_t * s, ulong cap ) {
  if( s->h_budget ) return FD_ED25519_AMD_OK;
  HIPCHK( hipHostMalloc( (void **)&s->h_budget, sizeof(fd_txn_amd_budget_t)*cap, hipHostMallocMapped | hipHostMallocCoherent ) );
  HIPCHK( hipHostGetDevicePointer( &s->m_budget, s->h_budget, 0 ) );
  return FD_ED25519_AMD_OK;
}

/* The slot's idle block and status plane, on its first frag submission.  The
   block is zeroed on the slot's stream, ahead of the kernels that read it. */
static int
slot_alloc_frags( slot_t * s, ulong cap ) {
  if( s->d_fpack ) return FD_ED25519_AMD_OK;
  HIPCHK( hipMalloc( (void **)&s->d_fpack, 256UL + cap ) );
  s->d_fstat = (int8_t *)(s->d_fpack + 256UL);
  HIPCHK( hipMemsetAsync( s->d_fpack, 0, 256UL, s->stream ) );
  return FD_ED25519_AMD_OK;
}

static_assert( FD_ED25519_AMD_VERDICT_FRAG_SEQ == FD_AMD_VERDICT_FRAG_SEQ && FD_ED25519_AMD_VERDICT_FRAG_BAD == FD_AMD_VERDICT_FRAG_BAD,
               "fd_ed25519_kernels.h restates these" );
static_assert( sizeof(fd_frag_meta_t) == 32UL && sizeof(fd_amd_gather_rec_t) == 32UL, "k_frag_list reads and writes 32-B records" );

static_assert( sizeof(fd_txn_amd_budget_t) == 24UL && alignof(fd_txn_amd_budget_t) == 8UL, "fd_amd_budget_record's three words" );
static_assert( FD_TXN_AMD_BUDGET_OK == FD_AMD_BUDGET_OK && FD_TXN_AMD_BUDGET_INVALID == FD_AMD_BUDGET_INVALID &&
               FD_TXN_AMD_BUDGET_NOPARSE == FD_AMD_BUDGET_NOPARSE && FD_TXN_AMD_BUDGET_FLAG_SET_CU == FD_AMD_BUDGET_F_CU &&
               FD_TXN_AMD_BUDGET_FLAG_SET_FEE == FD_AMD_BUDGET_F_FEE && FD_TXN_AMD_BUDGET_FLAG_SET_HEAP == FD_AMD_BUDGET_F_HEAP &&
               FD_TXN_AMD_BUDGET_FLAG_SET_TOTAL_FEE == FD_AMD_BUDGET_F_TOTAL, "fd_txn_budget.h restates these" );

/* The store kernel's wave cap in the engine: its stores go to host memory
   beside the other slots' kernels (slot_launch_gather's reason, the other
   way round). */
#define EMIT_WAVES (128u)

/* The filter step of both launch tails, for a _keep submission: the
   survivors of the chunk's n items, from their verdicts d_err (in the
   engine's mode: behind k_strict) and tags d_tag, both on the device, into
   the mapped h_keep / h_kcnt -- written in place by the filter's last
   kernels, as the verdicts are by slot_out.  fp / fpk: fd_amd_launch_keep's.
   With a window attached the step also filters against it and feeds it.
   Submissions act on the window in ticket order, which is the order of
   these calls: the window's kernels wait for the event the previous
   submission recorded behind its own (on another slot's stream; everything
   ahead of them still overlaps) and the slot's is recorded behind them. */
static int
slot_keep( slot_t * s, ulong n, int8_t const * d_err, ulong const * d_tag, uint32_t const * fp, uint32_t * fpk ) {
  fd_ed25519_amd_window_t * w = s->win_arm;
  if( !w )
    return fd_amd_launch_keep( (uint32_t)n, d_err, (uint64_t const *)d_tag, fp, fpk, (uint32_t *)s->m_keep, (uint64_t *)s->m_kcnt,
                               s->d_kscr, s->salt, s->stream ) ? FD_ED25519_AMD_ERR_DEVICE : FD_ED25519_AMD_OK;
  fd_amd_win_dev_t d = fd_amd_window_arm( w, n, s->win_done );
  return fd_amd_launch_keep_win( (uint32_t)n, d_err, (uint64_t const *)d_tag, fp, fpk, (uint32_t *)s->m_keep, (uint64_t *)s->m_kcnt,
                                 s->d_kscr, s->salt, &d, s->stream ) ? FD_ED25519_AMD_ERR_DEVICE : FD_ED25519_AMD_OK;
}

/* The n tags of the chunk just verified on s (the tag plane of its
   workspace) into h_tag, on the slot's stream: k_tag_out writes the mapped
   buffer, on every path, as slot_out does the verdicts and for its reason.
   A D2H copy of the plane instead, measured on the throughput path (a 2^20 x
   200 B verify_soa, 16 chunks): +2.2 to +2.6 ms per call, 9-10 %, behind the
   other slot's H2D; the kernel: within the untagged calls' spread
   (profiles/tag_copy_ab.txt). */
static int
slot_tags( slot_t * s, ulong n ) {
  return fd_amd_launch_tag_out( s->m_tag, s->d_ws, n, s->stream ) ? FD_ED25519_AMD_ERR_DEVICE : FD_ED25519_AMD_OK;
}

/* Forget the chunk in flight on s: where its outputs were to go, and that
   there is one.  A slot that is not busy has an all-zero record. */
static void
slot_forget( slot_t * s ) {
  memset( &s->fl, 0, sizeof(s->fl) );
  s->busy = 0;
}

/* Wait for a slot's chunk and deliver its verdicts and, where the caller
   asked for them, its tags and descriptors: one place, so that draining a
   slot before it is reused covers every output. */
static int
slot_drain( slot_t * s ) {
  if( !s->busy ) return FD_ED25519_AMD_OK;
  HIPCHK( hipEventSynchronize( s->done ) );
  slot_flight_t const & f = s->fl;
  /* k_dsmp's hang guard marks every verdict of its launch (k_fin) */
  bool fault = ( f.chk_err  && s->h_err[0] == (int8_t)FD_AMD_VERDICT_DEVICE ) ||
               ( f.chk_terr && memchr( s->h_terr, (uint8_t)FD_AMD_VERDICT_DEVICE, f.chk_terr ) );
  if( fault ) fprintf( stderr, "fd_ed25519_amd: the pooled double-scalar multiply hit its step guard\n" );
  /* descriptors: the chunk's total is known only now.  The callers' bound
     check keeps both conditions from ever holding; they are the backstop that
     keeps the copy below inside the staging and the caller's buffer */
  else if( f.do_out && ( s->h_doff[f.do_n] > s->desc_stage || *f.d_base + s->h_doff[f.do_n] > f.d_cap ) ) {
    fprintf( stderr, "fd_ed25519_amd: a chunk's descriptors exceed their bound\n" );
    fault = true;
  } else if( f.k_out && s->h_kcnt[0] > f.k_n ) {   /* the same backstop for the publish list */
    fprintf( stderr, "fd_ed25519_amd: a chunk's survivors exceed its items\n" );
    fault = true;
  } else if( f.e_off && s->h_eoff[s->h_kcnt[0]] > f.e_cap ) {   /* and for the frames (none was stored past the extent) */
    fprintf( stderr, "fd_ed25519_amd: a chunk's frames exceed their bound\n" );
    fault = true;
  } else {
    for( int k=0; k<f.ncp; k++ ) memcpy( f.cp[k].dst, f.cp[k].src, f.cp[k].sz );
    if( f.k_out ) {   /* keep[0, count) and the count; nothing at or beyond keep[count] */
      ulong const cnt = s->h_kcnt[0];
      if( cnt ) memcpy( f.k_out, s->h_keep, 4UL*cnt );
      *f.k_cnt = cnt;
      if( f.e_off ) {   /* emit_off[0 .. count] and emit_sz[0 .. count); nothing beyond them */
        memcpy( f.e_off, s->h_eoff, 8UL*(cnt + 1UL) );
        if( cnt ) memcpy( f.e_sz, s->h_esz, 4UL*cnt );
      }
    }
    if( f.do_out ) {   /* chunk-relative offsets -> the batch's numbering; the bytes behind the earlier chunks' */
      ulong const base = *f.d_base, tot = s->h_doff[f.do_n];
      for( ulong j=0; j<=f.do_n; j++ ) f.do_out[j] = base + s->h_doff[j];
      if( tot ) memcpy( f.d_out + base, s->h_desc, tot );
      *f.d_base = base + tot;
    }
  }
  slot_forget( s );
  return fault ? FD_ED25519_AMD_ERR_DEVICE : FD_ED25519_AMD_OK;
}

/* Error exit of a batch call: wait for every chunk still in flight and
   forget where its verdicts, tags and descriptors were to go, so no later
   call writes into the caller's (by then possibly freed) output arrays. */
static int
engine_quiesce( fd_ed25519_amd_t * e, int rc ) {
  for( int k=0; k<FD_AMD_SLOT_MAX; k++ ) {
    slot_t * s = &e->slot[k];
    if( s->busy ) (void)hipEventSynchronize( s->done );
    slot_forget( s );
  }
  e->a_cnt = 0; e->a_head = e->a_tail;   /* every submission in flight is dropped */
  return rc;
}

/* The end of every chunk's launch: the slot's event behind all of it.  A
   submission that polls its completion word has k_ticket store its ticket
   there first, the last kernel on the stream. */
static int
slot_done( slot_t * s ) {
  if( s->tick_arm && fd_amd_launch_ticket( s->m_tick, s->ticket, s->stream ) ) return FD_ED25519_AMD_ERR_DEVICE;
  HIPCHK( hipEventRecord( s->done, s->stream ) );
  return FD_ED25519_AMD_OK;
}

/* When the chunk being launched on s is drained, `sz` bytes of the slot's
   staging at src go to the caller's dst (NULL: not asked for). */
static void
slot_deliver( slot_t * s, void * dst, void const * src, ulong sz ) {
  if( dst ) s->fl.cp[s->fl.ncp++] = { dst, src, sz };
}

/* The five planes a chunk's verify kernels read, as the device sees them. */
struct planes_t { uint8_t const * pub; uint8_t const * sig; uint32_t const * off; uint32_t const * sz; uint8_t const * blob; };

static inline planes_t
slot_planes( slot_t const * s ) { return planes_t{ s->d_pub, s->d_sig, s->d_off, s->d_sz, s->d_blob }; }

/* The verify launch of every engine slot, into the slot's d_err and
   workspace on its stream, in the engine's mode.  skip and out: as
   fd_amd_launch_verify's d_skip and d_out. */
static int
slot_verify( slot_t * s, ulong n, planes_t const & p, int want_stats, int8_t const * skip, void * out ) {
  return fd_amd_launch_verify( (uint32_t)n, p.pub, p.sig, p.off, p.sz, p.blob, s->d_err, s->d_ws, s->stream, want_stats, NULL,
                               skip, 0, (int8_t *)out, s->strict ) ? FD_ED25519_AMD_ERR_DEVICE : FD_ED25519_AMD_OK;
}

/* The launch tail of every signature chunk: n signatures whose planes p are
   on the device (or on their way there on the slot's stream, or mapped) are
   verified; the n verdicts, written to h_err, go to `err` when the slot is
   drained; with tag != NULL the n tags, written to h_tag, go to `tag`. */
static int
slot_launch_sig( slot_t * s, ulong n, planes_t const & p, schar * err, ulong * tag ) {
  /* latency path: the DSM kernel (strict mode: k_strict) writes the verdicts
     into the mapped h_err itself */
  bool const lat = fd_amd_uses_latency_path( (uint32_t)n, 0 ) != 0;
  if( slot_verify( s, n, p, 1, NULL, lat ? s->m_err : NULL ) ) return FD_ED25519_AMD_ERR_DEVICE;
  /* a frag submission: the items' statuses over the verdicts and 0 over their tags, ahead of everything that
     reads either; on the latency path over the mapped verdicts too, which slot_out writes otherwise */
  if( s->frag_arm.mcache &&
      fd_amd_launch_frag_verdict( (uint32_t)n, s->d_fstat, s->frag_arm.mcache, s->frag_arm.depth, s->frag_arm.seq0, s->d_err,
                                  lat ? (int8_t *)s->m_err : NULL, s->d_ws, s->stream ) )
    return FD_ED25519_AMD_ERR_DEVICE;
  if( !lat ) HIPCHK( slot_out( s, s->m_err, s->d_err, n ) );
  /* latency path: k_tag_out after the DSM kernel.  The stream is in order
     and the host waits for one event behind both outputs, so either side of
     the DSM kernel costs the same one launch; after it, the verify launch
     sequence is the untagged call's */
  if( tag && slot_tags( s, n ) ) return FD_ED25519_AMD_ERR_DEVICE;
  /* survivors: the filter reads the verdicts and the workspace's tag plane where the verify left them */
  if( s->keep_arm && slot_keep( s, n, s->d_err, (ulong const *)((uint8_t const *)s->d_ws + fd_amd_ws_layout( n ).tag), NULL, NULL ) )
    return FD_ED25519_AMD_ERR_DEVICE;
  /* frames: behind k_keep_store, from the planes the verify kernels read and the survivors in the mapped h_keep */
  if( s->emit_arm.out &&
      fd_amd_launch_emit_sig( (uint32_t)n, p.pub, p.sig, p.off, p.sz, p.blob, (uint32_t const *)s->m_keep, (uint64_t const *)s->m_kcnt,
                              (void *)s->emit_arm.dev, s->emit_arm.cap, (uint64_t *)s->m_eoff, (uint32_t *)s->m_esz, s->d_epack,
                              EMIT_WAVES, s->stream ) )
    return FD_ED25519_AMD_ERR_DEVICE;
  if( slot_done( s ) ) return FD_ED25519_AMD_ERR_DEVICE;
  slot_deliver( s, err, s->h_err, n );
  slot_deliver( s, tag, s->h_tag, 8UL*n );
  s->fl.chk_err = n;
  s->fl.k_out = s->keep_arm; s->fl.k_cnt = s->kcnt_arm; s->fl.k_n = n;
  s->fl.e_off = s->emit_arm.out ? s->emit_arm.off : NULL; s->fl.e_sz = s->emit_arm.sz; s->fl.e_cap = s->emit_arm.cap;
  s->busy = 1;
  return FD_ED25519_AMD_OK;
}

/* Chunk of n signatures staged in s->h_pack as [pub 32n | sig 64n | off 4n | sz 4n | blob]. */
static int
slot_launch_packed( slot_t * s, ulong n, ulong blob_sz, schar * out, ulong * tag ) {
  /* latency path: k_front reads the staging in place over PCIe (one pass,
     ~300 B per signature), which saves the H2D and its launch gap; larger
     batches copy first (their kernels re-read the inputs) */
  uint8_t * d = s->m_pack;
  if( !fd_amd_uses_latency_path( (uint32_t)n, 0 ) ) {
    d = s->d_pack;
    HIPCHK( hipMemcpyAsync( d, s->h_pack, 104UL*n + blob_sz, hipMemcpyHostToDevice, s->stream ) );
  }
  return slot_launch_sig( s, n, planes_t{ d, d + 32UL*n, (uint32_t *)(d + 96UL*n), (uint32_t *)(d + 100UL*n), d + 104UL*n },
                          out, tag );
}

/* Where one transaction chunk's outputs go: the caller's arrays at the
   chunk's first transaction (txn_err, txn_tag, desc_off) and first signature
   slot (sig_err, sig_tag), NULL where not asked for; the whole descriptor
   buffer, and the call's running descriptor byte base; budget at the chunk's
   first transaction. */
struct txn_outs_t {
  schar * txn_err; schar * sig_err; ulong * txn_tag; ulong * sig_tag;
  ulong * desc_off; uchar * desc; ulong desc_cap; ulong * dbase;
  fd_txn_amd_budget_t * budget;   /* the chunk's first record (NULL: not asked for) */
};

/* The kernels of a transaction chunk whose payloads and planes (d_blob,
   d_toff, d_tsz, d_tbase[0..c]) are on the device, or on their way there on
   the slot's stream: parse, verify with d_skip, reduce, outputs, tags,
   descriptors.  c transactions, nslot = d_tbase[c] signature slots.
   Per-transaction verdicts land in h_terr, per-signature ones (when
   o.sig_err) in h_err; the per-transaction tags (when o.txn_tag) in h_ttag,
   the per-signature ones (when o.sig_tag) in h_tag; with o.desc_off the
   chunk's descriptors, packed, in h_desc and their chunk-relative offsets in
   h_doff[0..c] (desc_bound: the sum of fd_txn_amd_desc_bound over the
   chunk); with o.budget the chunk's compute budget records in h_budget. */
static int
slot_launch_txn_dev( slot_t * s, ulong c, ulong nslot, txn_outs_t const & o, ulong desc_bound ) {
  if( fd_amd_launch_txn_parse( (uint32_t)c, s->d_blob, s->d_toff, s->d_tsz, s->d_fp, NULL, 0, s->d_tbase,
                               s->d_pub, s->d_sig, s->d_off, s->d_sz, s->d_skip, s->stream ) )
    return FD_ED25519_AMD_ERR_DEVICE;
  /* compute budget: needs the payloads and the footprints alone, so it goes
     right behind the parse (ahead of the verify kernels and of the stretch a
     window serialises) and writes the mapped h_budget in place, as
     k_tag_gather does h_ttag */
  if( o.budget && fd_amd_launch_txn_budget( (uint32_t)c, s->d_blob, s->d_toff, s->d_tsz, s->d_fp, s->m_budget, s->stream ) )
    return FD_ED25519_AMD_ERR_DEVICE;
  if( nslot && slot_verify( s, nslot, slot_planes( s ), 0, s->d_skip, NULL ) ) return FD_ED25519_AMD_ERR_DEVICE;
  /* after k_strict (same stream): a transaction's verdict is its first failing signature's code in the engine's mode */
  if( fd_amd_launch_txn_reduce( (uint32_t)c, s->d_fp, s->d_tbase, s->d_err, s->d_terr, s->stream ) )
    return FD_ED25519_AMD_ERR_DEVICE;
  HIPCHK( slot_out( s, s->m_terr, s->d_terr, c ) );
  if( o.sig_err && nslot ) HIPCHK( slot_out( s, s->m_err, s->d_err, nslot ) );
  /* tags: per transaction its first slot's (no slot launched: no workspace is read), per signature the plane */
  if( o.txn_tag && fd_amd_launch_tag_gather( s->m_ttag, s->d_ws, (uint32_t)c, s->d_tbase, s->stream ) ) return FD_ED25519_AMD_ERR_DEVICE;
  if( o.sig_tag && nslot && slot_tags( s, nslot ) ) return FD_ED25519_AMD_ERR_DEVICE;
  /* descriptors: packed in HBM from the footprints k_txn_parse left (0 where
     it rejected the payload, the fail-closed slot mismatch included), then
     one coalesced copy-out that reads the chunk's total on the device: the
     host learns it from h_doff[c] when it drains the slot, without a sync */
  /* survivors: the filter over the per-transaction verdicts and the tags of
     the transactions' first slots, gathered into a device plane (not read
     back from the mapped h_ttag); with descriptors it also leaves the masked
     footprints, and the pack below runs on those: descriptors for survivors only */
  /* frames need the survivors' packed descriptors on the device, asked for or
     not: the pack then runs (on the masked footprints) and k_desc_out does not */
  bool const emit = s->emit_arm.out != NULL, pack = o.desc_off || emit;
  uint32_t const * fp = s->d_fp;
  if( s->keep_arm ) {
    if( fd_amd_launch_tag_gather( s->d_ktag, s->d_ws, (uint32_t)c, s->d_tbase, s->stream ) ||
        slot_keep( s, c, s->d_terr, s->d_ktag, pack ? s->d_fp : NULL, pack ? s->d_fpk : NULL ) )
      return FD_ED25519_AMD_ERR_DEVICE;
    fp = s->d_fpk;
  }
  if( pack && fd_amd_launch_txn_pack( (uint32_t)c, s->d_blob, s->d_toff, s->d_tsz, fp, s->d_dbsum, s->d_doff, s->d_desc,
                                      s->desc_stage, s->stream ) )
    return FD_ED25519_AMD_ERR_DEVICE;
  if( o.desc_off &&
      fd_amd_launch_desc_out( s->m_desc, s->d_desc, s->m_doff, s->d_doff, (uint32_t)c, s->desc_stage, desc_bound, s->stream ) )
    return FD_ED25519_AMD_ERR_DEVICE;
  if( emit &&
      fd_amd_launch_emit_txn( (uint32_t)c, s->d_blob, s->d_toff, s->d_tsz, (uint64_t const *)s->d_doff, s->d_desc,
                              (uint32_t const *)s->m_keep, (uint64_t const *)s->m_kcnt, (void *)s->emit_arm.dev, s->emit_arm.cap,
                              (uint64_t *)s->m_eoff, (uint32_t *)s->m_esz, s->d_epack, EMIT_WAVES, s->stream ) )
    return FD_ED25519_AMD_ERR_DEVICE;
  if( slot_done( s ) ) return FD_ED25519_AMD_ERR_DEVICE;
  slot_deliver( s, o.txn_err, s->h_terr, c );
  slot_deliver( s, o.txn_tag, s->h_ttag, 8UL*c );
  slot_deliver( s, o.budget, s->h_budget, sizeof(fd_txn_amd_budget_t)*c );
  if( nslot ) {
    slot_deliver( s, o.sig_err, s->h_err, nslot );
    slot_deliver( s, o.sig_tag, s->h_tag, 8UL*nslot );
  }
  s->fl.chk_err = (o.sig_err && nslot) ? nslot : 0; s->fl.chk_terr = c;
  s->fl.do_out = o.desc_off; s->fl.do_n = c;
  s->fl.d_out = o.desc; s->fl.d_cap = o.desc_cap; s->fl.d_base = o.dbase;
  s->fl.k_out = s->keep_arm; s->fl.k_cnt = s->kcnt_arm; s->fl.k_n = c;
  s->fl.e_off = emit ? s->emit_arm.off : NULL; s->fl.e_sz = s->emit_arm.sz; s->fl.e_cap = s->emit_arm.cap;
  s->busy = 1;
  return FD_ED25519_AMD_OK;
}

/* Launch a staged transaction chunk: c transactions (payload bytes in
   h_blob, rebased offsets in h_toff/h_tsz, signature-slot bases in
   h_tbase[0..c]), nslot = h_tbase[c] signature slots. */
static int
slot_launch_txn( slot_t * s, ulong c, ulong nslot, ulong blob_sz, txn_outs_t const & o, ulong desc_bound ) {
  HIPCHK( hipMemcpyAsync( s->d_toff,  s->h_toff,  4UL*c,        hipMemcpyHostToDevice, s->stream ) );
  HIPCHK( hipMemcpyAsync( s->d_tsz,   s->h_tsz,   4UL*c,        hipMemcpyHostToDevice, s->stream ) );
  HIPCHK( hipMemcpyAsync( s->d_tbase, s->h_tbase, 4UL*(c+1UL),  hipMemcpyHostToDevice, s->stream ) );
  if( blob_sz ) HIPCHK( hipMemcpyAsync( s->d_blob, s->h_blob, blob_sz, hipMemcpyHostToDevice, s->stream ) );
  return slot_launch_txn_dev( s, c, nslot, o, desc_bound );
}

/* The chunk driver of every host batch call: `total` items (signatures or
   transactions) go through slots [0, ring) round robin.  A slot's previous
   chunk is drained before the slot is reused; stage( slot, first ) sizes,
   stages and launches the chunk that starts at item `first` and returns the
   items it took (> 0; the callers' argument checks see to that) or an error
   code (< 0); the ring is drained at the end, in the order the chunks were
   launched, as the loop drains them.  Any error quiesces the engine. */
template<typename STAGE>
static int
run_ring( fd_ed25519_amd_t * e, int ring, ulong total, STAGE stage ) {
  if( hipSetDevice( e->device ) != hipSuccess ) return FD_ED25519_AMD_ERR_DEVICE;
  int rc; int k = 0;
  for( ulong i=0; i<total; k=(k + 1) % ring ) {
    slot_t * s = &e->slot[k];
    if( (rc = slot_drain( s )) ) return engine_quiesce( e, rc );
    long c = stage( s, i );
    if( c < 0L ) return engine_quiesce( e, (int)c );
    i += (ulong)c;
  }
  /* oldest chunk first: slot k is the one the next chunk would have reused
     (a chunk's descriptors are placed behind those of every earlier chunk) */
  for( int j=0; j<ring; j++ ) if( (rc = slot_drain( &e->slot[(k + j) % ring] )) ) return engine_quiesce( e, rc );
  return FD_ED25519_AMD_OK;
}

/* Submissions in flight hold slots the synchronous calls (and a mode change)
   would reuse: those refuse, before they touch anything. */
#define SYNC_REFUSED( e ) ( (e) && (e)->a_cnt )

/* The argument check of the staged pointer-array calls. */
static int
batch_args_check( fd_ed25519_amd_t const * e, ulong n, void const * const * msg, ulong const * sz,
                  void const * const * sig, void const * const * pub, schar const * err ) {
  if( !e || (n && (!msg || !sz || !sig || !pub || !err)) ) return FD_ED25519_AMD_ERR_INVAL;
  for( ulong j=0; j<n; j++ )            /* every message must fit one chunk: checked before anything launches */
    if( sz[j] > e->blob_cap || (sz[j] && !msg[j]) ) return FD_ED25519_AMD_ERR_INVAL;
  return FD_ED25519_AMD_OK;
}

/* The chunk the staged pointer-array call cuts off the front of n signatures. */
static ulong
batch_chunk( fd_ed25519_amd_t const * e, ulong n, ulong const * sz ) {
  ulong c = 0, bsz = 0;
  while( c < n && c < e->cap && bsz + sz[c] <= e->blob_cap ) { bsz += sz[c]; c++; }
  return c;
}

/* Stage and launch on s the first chunk of the n signatures given (the
   arrays start at the chunk's first signature); returns the signatures
   taken or an error code. */
static long
stage_batch( fd_ed25519_amd_t * e, slot_t * s, ulong n, void const * const * msg, ulong const * sz,
             void const * const * sig, void const * const * pub, schar * err, ulong * tag ) {
  if( tag ) { int rc = slot_alloc_tag( s, e->cap ); if( rc ) return rc; }
  /* size the chunk first, then stage it packed: [pub|sig|off|sz|blob] */
  ulong const c = batch_chunk( e, n, sz );
  uint8_t * hp = s->h_pack;
  uint8_t * h_pub = hp, * h_sig = hp + 32UL*c, * h_blob = hp + 104UL*c;
  uint32_t * h_off = (uint32_t *)(hp + 96UL*c), * h_sz = (uint32_t *)(hp + 100UL*c);
  ulong bsz = 0;
  for( ulong j=0; j<c; j++ ) {
    memcpy( h_pub + 32UL*j, pub[j], 32 );
    memcpy( h_sig + 64UL*j, sig[j], 64 );
    if( sz[j] ) memcpy( h_blob + bsz, msg[j], sz[j] );
    h_off[j] = (uint32_t)bsz; h_sz[j] = (uint32_t)sz[j];
    bsz += sz[j];
  }
  int rc = slot_launch_packed( s, c, bsz, err, tag );
  return rc ? rc : (long)c;
}

extern "C" int
fd_ed25519_amd_verify_batch( fd_ed25519_amd_t * e, ulong n, void const * const * msg, ulong const * sz,
                             void const * const * sig, void const * const * pub, schar * err ) {
  return fd_ed25519_amd_verify_batch_tag( e, n, msg, sz, sig, pub, err, NULL );
}

extern "C" int
fd_ed25519_amd_verify_batch_tag( fd_ed25519_amd_t * e, ulong n, void const * const * msg, ulong const * sz,
                                 void const * const * sig, void const * const * pub, schar * err, ulong * tag ) {
  if( SYNC_REFUSED( e ) ) return FD_ED25519_AMD_ERR_INVAL;
  int rc = batch_args_check( e, n, msg, sz, sig, pub, err );
  if( rc ) return rc;
  return run_ring( e, 2, n, [&]( slot_t * s, ulong i ) -> long {
    return stage_batch( e, s, n - i, msg + i, sz + i, sig + i, pub + i, err + i, tag ? tag + i : NULL );
  } );
}

/* memcpy split over up to 4 host threads for large copies (the staging
   copy is the host-side limit of the SoA path: ~300 B per signature). */
static void
copy_par( void * dst, void const * src, ulong sz ) {
  ulong const min_part = 4UL << 20;
  int nt = (int)( sz / min_part ); if( nt > 4 ) nt = 4;
  if( nt < 2 ) { if( sz ) memcpy( dst, src, sz ); return; }
  std::thread th[3];
  ulong part = ( sz / (ulong)nt + 63UL ) & ~63UL;
  for( int t=1; t<nt; t++ ) {
    ulong lo = part*(ulong)t, hi = lo + part < sz ? lo + part : sz;
    if( lo < hi ) th[t-1] = std::thread( [=]{ memcpy( (uint8_t *)dst + lo, (uint8_t const *)src + lo, hi - lo ); } );
  }
  memcpy( dst, src, part < sz ? part : sz );
  for( int t=1; t<nt; t++ ) if( th[t-1].joinable() ) th[t-1].join();
}

int
fd_amd_soa_args_check( fd_ed25519_amd_t const * e, ulong n, uchar const * pub, uchar const * sig, uint const * msg_off,
                       uint const * msg_sz, uchar const * blob, ulong blob_sz, schar const * err ) {
  if( !e || (n && (!pub || !sig || !msg_off || !msg_sz || !err)) ) return FD_ED25519_AMD_ERR_INVAL;
  for( ulong i=0; i<n; i++ )
    if( msg_sz[i] && ((ulong)msg_off[i] + msg_sz[i] > blob_sz || !blob || msg_sz[i] > e->blob_cap) )
      return FD_ED25519_AMD_ERR_INVAL;
  return FD_ED25519_AMD_OK;
}

/* One SoA chunk: c signatures from signature i on (up to cap, and blob_cap
   message bytes), their bsz message bytes, and the window [lo, lo+win) of
   the blob those span (0, 0: no message bytes).  fit_window: also end the
   chunk before its window outgrows blob_cap (the registered path copies the
   window whole into d_blob). */
struct soa_chunk_t { ulong c, bsz, lo, win; };

static soa_chunk_t
soa_chunk( fd_ed25519_amd_t const * e, ulong n, ulong i, uint const * msg_off, uint const * msg_sz, bool fit_window ) {
  ulong c = 0, bsz = 0, lo = ~0UL, hi = 0UL;
  while( i + c < n && c < e->cap ) {
    ulong sz = msg_sz[i+c];                  /* <= blob_cap: fd_amd_soa_args_check */
    if( bsz + sz > e->blob_cap ) break;
    if( sz ) {
      ulong o = msg_off[i+c];
      ulong nlo = o < lo ? o : lo, nhi = o + sz > hi ? o + sz : hi;
      if( fit_window && nhi - nlo > e->blob_cap ) break;
      lo = nlo; hi = nhi;
    }
    bsz += sz; c++;
  }
  return hi > lo ? soa_chunk_t{ c, bsz, lo, hi - lo } : soa_chunk_t{ c, bsz, 0UL, 0UL };
}

/* Stage chunk ch (pub, sig, msg_off, msg_sz: its first signature's) packed
   in s->h_pack; returns the blob bytes staged.  pub and sig are contiguous
   per chunk: block copies.  window: the chunk's window of the blob is
   copied as one block and the offsets rebased (no per-message copy); else
   the messages are gathered one by one. */
static ulong
soa_stage( slot_t * s, soa_chunk_t ch, uchar const * pub, uchar const * sig, uint const * msg_off, uint const * msg_sz,
           uchar const * blob, bool window ) {
  ulong c = ch.c;
  uint8_t * hp = s->h_pack;
  uint8_t * h_blob = hp + 104UL*c;
  uint32_t * h_off = (uint32_t *)(hp + 96UL*c), * h_sz = (uint32_t *)(hp + 100UL*c);
  copy_par( hp, pub, 32UL*c );
  copy_par( hp + 32UL*c, sig, 64UL*c );
  memcpy( h_sz, msg_sz, 4UL*c );
  if( window ) {
    copy_par( h_blob, blob + ch.lo, ch.win );
    for( ulong j=0; j<c; j++ ) h_off[j] = msg_sz[j] ? (uint32_t)(msg_off[j] - ch.lo) : 0U;
    return ch.win;
  }
  ulong b = 0;
  for( ulong j=0; j<c; j++ ) {
    ulong sz = msg_sz[j];
    if( sz ) memcpy( h_blob + b, blob + msg_off[j], sz );
    h_off[j] = (uint32_t)b; b += sz;
  }
  return b;
}

/* SoA staging: a chunk whose messages sit in a window of the blob not much
   larger than their total size takes the block copy, other layouts the
   gather. */
extern "C" int
fd_ed25519_amd_verify_soa( fd_ed25519_amd_t * e, ulong n, uchar const * pub, uchar const * sig,
                           uint const * msg_off, uint const * msg_sz, uchar const * blob, ulong blob_sz,
                           schar * err ) {
  return fd_ed25519_amd_verify_soa_tag( e, n, pub, sig, msg_off, msg_sz, blob, blob_sz, err, NULL );
}

extern "C" int
fd_ed25519_amd_verify_soa_tag( fd_ed25519_amd_t * e, ulong n, uchar const * pub, uchar const * sig,
                               uint const * msg_off, uint const * msg_sz, uchar const * blob, ulong blob_sz,
                               schar * err, ulong * tag ) {
  if( SYNC_REFUSED( e ) ) return FD_ED25519_AMD_ERR_INVAL;
  int rc = fd_amd_soa_args_check( e, n, pub, sig, msg_off, msg_sz, blob, blob_sz, err );
  if( rc ) return rc;
  return run_ring( e, e->nslot, n, [&]( slot_t * s, ulong i ) -> long {
    if( tag ) { int rc = slot_alloc_tag( s, e->cap ); if( rc ) return rc; }
    soa_chunk_t ch = soa_chunk( e, n, i, msg_off, msg_sz, false );
    bool window = ch.win <= e->blob_cap && ch.win <= ch.bsz + ch.bsz/4UL + 4096UL;
    ulong b = soa_stage( s, ch, pub + 32UL*i, sig + 64UL*i, msg_off + i, msg_sz + i, blob, window );
    int rc = slot_launch_packed( s, ch.c, b, err + i, tag ? tag + i : NULL );
    return rc ? rc : (long)ch.c;
  } );
}

/* ------------------------------------------------------------------ */
/* zero-copy host batches (caller memory registered once)               */

/* Registrations made through fd_ed25519_amd_host_register, with their
   device addresses: the latency path validates and translates a plane with
   a table lookup instead of four HIP pointer queries per plane (~25 runtime
   calls per batch of five planes, most of the host-side overhead of a
   0.5 ms call).  Memory registered by other means takes the query path. */
namespace {
struct reg_t { uintptr_t lo, hi; uintptr_t dev; };
std::mutex          g_reg_mu;
std::vector<reg_t>  g_reg;
}

extern "C" int
fd_ed25519_amd_host_register( void * base, ulong sz ) {
  if( !base || !sz ) return FD_ED25519_AMD_ERR_INVAL;
  /* portable: usable by every device's engine; mapped: small batches are
     read in place by the GPU (no copy at all) */
  if( hipHostRegister( base, sz, hipHostRegisterPortable | hipHostRegisterMapped ) != hipSuccess )
    return FD_ED25519_AMD_ERR_DEVICE;
  void * dev = NULL;
  if( hipHostGetDevicePointer( &dev, base, 0 ) == hipSuccess ) {
    std::lock_guard<std::mutex> g( g_reg_mu );
    g_reg.push_back( reg_t{ (uintptr_t)base, (uintptr_t)base + sz, (uintptr_t)dev } );
  } else (void)hipGetLastError();
  return FD_ED25519_AMD_OK;
}

extern "C" int
fd_ed25519_amd_host_unregister( void * base ) {
  if( !base ) return FD_ED25519_AMD_ERR_INVAL;
  {
    std::lock_guard<std::mutex> g( g_reg_mu );
    for( size_t k=0; k<g_reg.size(); k++ )
      if( g_reg[k].lo == (uintptr_t)base ) { g_reg[k] = g_reg.back(); g_reg.pop_back(); break; }
  }
  return hipHostUnregister( base ) == hipSuccess ? FD_ED25519_AMD_OK : FD_ED25519_AMD_ERR_DEVICE;
}

/* [p, p+sz) lies in ONE registration: its first and its last byte are
   registered host memory and map to device addresses sz-1 apart (two
   adjacent registrations map to unrelated device ranges).  The latency
   path reads the planes in place, so a plane registered only in part must
   be refused here, not faulted on by the GPU.  *dev: p's device address. */
static bool
host_registered( void const * p, ulong sz, void ** dev ) {
  {
    std::lock_guard<std::mutex> g( g_reg_mu );
    uintptr_t const a = (uintptr_t)p, b = a + (sz ? sz : 1UL);
    for( reg_t const & r : g_reg )
      if( a >= r.lo && b <= r.hi && b > a ) { *dev = (void *)(r.dev + (a - r.lo)); return true; }
  }
  hipPointerAttribute_t a;
  if( hipPointerGetAttributes( &a, p ) != hipSuccess ) { (void)hipGetLastError(); return false; }
  if( a.type != hipMemoryTypeHost ) return false;
  void * dp = NULL, * dq = NULL;
  if( hipHostGetDevicePointer( &dp, (void *)p, 0 ) != hipSuccess ) { (void)hipGetLastError(); return false; }
  *dev = dp;
  if( sz <= 1UL ) return true;
  void const * q = (uchar const *)p + (sz - 1UL);
  if( hipPointerGetAttributes( &a, q ) != hipSuccess ) { (void)hipGetLastError(); return false; }
  if( a.type != hipMemoryTypeHost ) return false;
  if( hipHostGetDevicePointer( &dq, (void *)q, 0 ) != hipSuccess ) { (void)hipGetLastError(); return false; }
  return (ulong)((uchar const *)dq - (uchar const *)dp) == sz - 1UL;
}

/* One chunk straight from registered caller memory: the pub/sig/off/sz
   slices and the message window [lo, lo+win) by DMA into the slot's
   device planes, offsets rebased on the device. */
static int
slot_launch_dma( slot_t * s, ulong c, uchar const * pub, uchar const * sig, uint const * off, uint const * sz,
                 uchar const * win_src, ulong win, uint lo, schar * out, ulong * tag ) {
  HIPCHK( hipMemcpyAsync( s->d_pub, pub, 32UL*c, hipMemcpyHostToDevice, s->stream ) );
  HIPCHK( hipMemcpyAsync( s->d_sig, sig, 64UL*c, hipMemcpyHostToDevice, s->stream ) );
  HIPCHK( hipMemcpyAsync( s->d_off, off, 4UL*c,  hipMemcpyHostToDevice, s->stream ) );
  HIPCHK( hipMemcpyAsync( s->d_sz,  sz,  4UL*c,  hipMemcpyHostToDevice, s->stream ) );
  if( win ) HIPCHK( hipMemcpyAsync( s->d_blob, win_src, win, hipMemcpyHostToDevice, s->stream ) );
  if( fd_amd_launch_rebase_off( (uint32_t)c, s->d_off, s->d_sz, lo, s->stream ) ) return FD_ED25519_AMD_ERR_DEVICE;
  return slot_launch_sig( s, c, slot_planes( s ), out, tag );
}

extern "C" int
fd_ed25519_amd_verify_soa_registered( fd_ed25519_amd_t * e, ulong n, uchar const * pub, uchar const * sig,
                                      uint const * msg_off, uint const * msg_sz, uchar const * blob, ulong blob_sz,
                                      schar * err ) {
  return fd_ed25519_amd_verify_soa_registered_tag( e, n, pub, sig, msg_off, msg_sz, blob, blob_sz, err, NULL );
}

extern "C" int
fd_ed25519_amd_verify_soa_registered_tag( fd_ed25519_amd_t * e, ulong n, uchar const * pub, uchar const * sig,
                                          uint const * msg_off, uint const * msg_sz, uchar const * blob, ulong blob_sz,
                                          schar * err, ulong * tag ) {
  if( SYNC_REFUSED( e ) ) return FD_ED25519_AMD_ERR_INVAL;
  int rc = fd_amd_soa_args_check( e, n, pub, sig, msg_off, msg_sz, blob, blob_sz, err );
  if( rc ) return rc;
  if( !n ) return FD_ED25519_AMD_OK;
  void * d[5] = { NULL, NULL, NULL, NULL, NULL };   /* the planes' device addresses */
  if( !host_registered( pub, 32UL*n, &d[0] ) || !host_registered( sig, 64UL*n, &d[1] ) ||
      !host_registered( msg_off, 4UL*n, &d[2] ) || !host_registered( msg_sz, 4UL*n, &d[3] ) ||
      (blob && blob_sz && !host_registered( blob, blob_sz, &d[4] )) )
    return FD_ED25519_AMD_ERR_INVAL;
  if( !(blob && blob_sz) ) d[4] = d[0];   /* no message bytes: any valid address */
  if( n <= e->cap && fd_amd_uses_latency_path( (uint32_t)n, 0 ) )
    /* a latency-path batch is read once, by k_front: it reads the caller's
       registered planes in place over PCIe, with no copy on either side (the
       verdicts go out in place too: slot_launch_sig) -- one chunk on a ring
       of one slot */
    return run_ring( e, 1, n, [&]( slot_t * s, ulong ) -> long {
      if( tag ) { int rc = slot_alloc_tag( s, e->cap ); if( rc ) return rc; }
      planes_t const p = { (uint8_t const *)d[0], (uint8_t const *)d[1], (uint32_t const *)d[2], (uint32_t const *)d[3],
                           (uint8_t const *)d[4] };
      int rc = slot_launch_sig( s, n, p, err, tag );
      return rc ? rc : (long)n;
    } );
  return run_ring( e, e->nslot, n, [&]( slot_t * s, ulong i ) -> long {
    if( tag ) { int rc = slot_alloc_tag( s, e->cap ); if( rc ) return rc; }
    soa_chunk_t ch = soa_chunk( e, n, i, msg_off, msg_sz, true );
    ulong * const tg = tag ? tag + i : NULL;
    int rc;
    if( ch.win <= ch.bsz + ch.bsz/4UL + 4096UL )
      rc = slot_launch_dma( s, ch.c, pub + 32UL*i, sig + 64UL*i, msg_off + i, msg_sz + i, blob + ch.lo, ch.win,
                            (uint)ch.lo, err + i, tg );
    else   /* scattered messages: gather them through the pinned staging */
      rc = slot_launch_packed( s, ch.c, soa_stage( s, ch, pub + 32UL*i, sig + 64UL*i, msg_off + i, msg_sz + i, blob, false ),
                               err + i, tg );
    return rc ? rc : (long)ch.c;
  } );
}

/* ------------------------------------------------------------------ */
/* pointer-array batches gathered by the GPU from registered memory     */

/* The one place that sizes a gathered chunk: of n signatures with message
   sizes sz[], a chunk takes the first (every message fits a chunk: the
   callers check sz <= blob_max up front) and further ones while their
   count stays <= cap and the padded total, the sum of round_up( sz, 16 ),
   stays <= blob_cap.  dst[j]: message j's offset in the chunk's blob, a
   multiple of 16; it owns [dst[j], dst[j] + round_up( sz[j], 16 )).
   Returns the signatures taken.  Pure host code. */
extern "C" ulong
fd_ed25519_amd_gather_layout( ulong n, ulong const * sz, ulong cap, ulong blob_cap, uint * dst ) {
  ulong c = 0, b = 0;
  while( c < n ) {
    ulong const pad = (sz[c] + 15UL) & ~15UL;
    if( c && ( c >= cap || sz[c] > blob_cap || b + pad > blob_cap ) ) break;
    dst[c] = (uint)b;
    b += pad; c++;
  }
  return c;
}

namespace {
/* The registration table as one call sees it: copied under g_reg_mu once,
   then searched without the lock, the last hit first (the frags of one
   dcache all lie in one registration). */
struct reg_view_t {
  std::vector<reg_t> reg;
  size_t             last = 0;
  reg_view_t() { std::lock_guard<std::mutex> g( g_reg_mu ); reg = g_reg; }
  /* [p, p+sz), sz > 0, lies in one registration of the table: *dev = p's device address */
  bool xlat( void const * p, ulong sz, uint64_t * dev ) {
    uintptr_t const a = (uintptr_t)p, b = a + sz;
    if( b <= a || reg.empty() ) return false;
    reg_t const * r = &reg[last];
    if( !( a >= r->lo && b <= r->hi ) ) {
      size_t k = 0;
      while( k < reg.size() && !( a >= reg[k].lo && b <= reg[k].hi ) ) k++;
      if( k == reg.size() ) return false;
      last = k; r = &reg[k];
    }
    *dev = (uint64_t)(r->dev + (a - r->lo));
    return true;
  }
  bool rec( fd_amd_gather_rec_t * o, void const * pub, void const * sig, void const * msg, ulong sz ) {
    o->msg = 0UL; o->sz = (uint32_t)sz;
    return pub && sig && xlat( pub, 32UL, &o->pub ) && xlat( sig, 64UL, &o->sig ) && ( !sz || ( msg && xlat( msg, sz, &o->msg ) ) );
  }
};
}

/* Chunk of c signatures whose records sit in s->h_pack: k_gather fetches
   them into the slot's planes, then slot_launch_sig on those.  The
   records reach the kernel in place (it reads the mapped h_pack, 32 B per
   signature, once) or, with copy, by one H2D into d_pack. */
static int
slot_launch_gather( slot_t * s, ulong c, bool copy, schar * out, ulong * tag ) {
  fd_amd_gather_rec_t const * d_rec = (fd_amd_gather_rec_t const *)s->m_pack;
  if( copy ) {
    HIPCHK( hipMemcpyAsync( s->d_pack, s->h_pack, 32UL*c, hipMemcpyHostToDevice, s->stream ) );
    d_rec = (fd_amd_gather_rec_t const *)s->d_pack;
  }
  bool const lat = fd_amd_uses_latency_path( (uint32_t)c, 0 ) != 0;
  /* A throughput chunk's gather runs beside the other slot's verify kernels,
     and its reads of host memory, while on their way, hold up those kernels'
     own memory traffic: 2^20 x 200 B in 16 chunks took 32.5 ms with one wave
     per 16 records (4096 waves a chunk), 29.6 at 256 waves, 26.0 at 128, 23.4
     at 64, 28.9 at 32 (a lone 2^16 chunk: 2.2-2.3 ms down to 64 waves, 2.5 at
     32: 64 waves still keep the link busy).  A latency-path batch is one
     chunk with nothing beside it: no cap. */
  if( fd_amd_launch_gather( (uint32_t)c, d_rec, s->d_pub, s->d_sig, s->d_off, s->d_sz, s->d_blob, lat ? 0u : 64u, s->stream ) )
    return FD_ED25519_AMD_ERR_DEVICE;
  return slot_launch_sig( s, c, slot_planes( s ), out, tag );
}

/* check( lo, hi ) over [0, n), true when it holds on every part.  The
   registered calls' up-front pass reads a pointer, a size and at most one
   payload byte per item and nothing of it overlaps the GPU: large batches
   (2^18 items and up) split it over up to 4 host threads, as copy_par does
   the staging copies. */
template<typename CHECK>
static bool
check_par( ulong n, CHECK check ) {
  int nt = (int)( n >> 17 ); if( nt > 4 ) nt = 4;
  if( nt < 2 ) return check( 0UL, n );
  std::thread th[3]; bool ok[4];
  ulong const part = ( n + (ulong)nt - 1UL ) / (ulong)nt;
  for( int t=1; t<nt; t++ ) th[t-1] = std::thread( [&, t]{ ok[t] = check( part*(ulong)t, std::min( n, part*(ulong)(t+1) ) ); } );
  ok[0] = check( 0UL, part );
  for( int t=1; t<nt; t++ ) th[t-1].join();
  for( int t=0; t<nt; t++ ) if( !ok[t] ) return false;
  return true;
}

/* Every signature of a registered pointer-array batch, before anything
   launches: its pointers, its size, and the first and last byte of each
   range in one registration of the table (32 B of pointers and sizes read
   per signature).  True when all pass. */
static bool
batch_registered_check( fd_ed25519_amd_t const * e, reg_view_t const & view, ulong n, void const * const * msg,
                        ulong const * sz, void const * const * sig, void const * const * pub ) {
  return check_par( n, [&]( ulong lo, ulong hi ) -> bool {
    reg_view_t v = view;                     /* its own last-hit index */
    fd_amd_gather_rec_t probe;
    for( ulong j=lo; j<hi; j++ )
      if( sz[j] > e->blob_cap || !v.rec( &probe, pub[j], sig[j], msg[j], sz[j] ) ) return false;
    return true;
  } );
}

/* Where a slot keeps a gathered chunk's dst offsets: behind its records in
   h_pack. */
static inline uint *
slot_gather_dst( fd_ed25519_amd_t const * e, slot_t * s ) { return (uint *)(s->h_pack + 32UL*e->cap); }

/* Stage and launch on s the first chunk of the n registered signatures given
   (the arrays start at the chunk's first signature); returns the signatures
   taken or an error code. */
static long
stage_batch_registered( fd_ed25519_amd_t * e, slot_t * s, reg_view_t & view, ulong n, void const * const * msg,
                        ulong const * sz, void const * const * sig, void const * const * pub, schar * err, ulong * tag ) {
  if( tag ) { int rc = slot_alloc_tag( s, e->cap ); if( rc ) return rc; }
  /* the chunk's records in h_pack (32 B per signature), their dst behind them */
  fd_amd_gather_rec_t * rec = (fd_amd_gather_rec_t *)s->h_pack;
  uint * dst = slot_gather_dst( e, s );
  ulong c = fd_ed25519_amd_gather_layout( n, sz, e->cap, e->blob_cap, dst );
  for( ulong j=0; j<c; j++ ) {
    /* translated again, not kept from the check: the chunk's translation
       runs beside the previous chunk's kernels, a table of n records would
       not; an address the table does not give never reaches the kernel */
    if( sz[j] > e->blob_cap || !view.rec( rec + j, pub[j], sig[j], msg[j], sz[j] ) ) return FD_ED25519_AMD_ERR_INVAL;
    rec[j].dst = dst[j];
  }
  int rc = slot_launch_gather( s, c, e->gather_copy != 0, err, tag );
  return rc ? rc : (long)c;
}

extern "C" int
fd_ed25519_amd_verify_batch_registered( fd_ed25519_amd_t * e, ulong n, void const * const * msg, ulong const * sz,
                                        void const * const * sig, void const * const * pub, schar * err ) {
  return fd_ed25519_amd_verify_batch_registered_tag( e, n, msg, sz, sig, pub, err, NULL );
}

extern "C" int
fd_ed25519_amd_verify_batch_registered_tag( fd_ed25519_amd_t * e, ulong n, void const * const * msg, ulong const * sz,
                                            void const * const * sig, void const * const * pub, schar * err,
                                            ulong * tag ) {
  if( SYNC_REFUSED( e ) ) return FD_ED25519_AMD_ERR_INVAL;
  if( !e || (n && (!msg || !sz || !sig || !pub || !err)) ) return FD_ED25519_AMD_ERR_INVAL;
  if( !n ) return FD_ED25519_AMD_OK;
  reg_view_t view;
  if( !batch_registered_check( e, view, n, msg, sz, sig, pub ) ) return FD_ED25519_AMD_ERR_INVAL;
  return run_ring( e, e->nslot, n, [&]( slot_t * s, ulong i ) -> long {
    return stage_batch_registered( e, s, view, n - i, msg + i, sz + i, sig + i, pub + i, err + i, tag ? tag + i : NULL );
  } );
}

/* Signature slots the engine reserves for a payload: its first byte when
   that is a plausible signature count (fd_txn_parse.c:79-82 accept it),
   else 0.  Exact for every payload that parses. */
ulong
fd_amd_txn_slots1( uchar const * p, ulong sz ) {
  if( !sz ) return 0UL;
  ulong k = p[0];
  return ( k >= 1UL && k <= FD_TXN_SIG_MAX && 64UL*k <= sz - 1UL ) ? k : 0UL;
}

extern "C" int
fd_ed25519_amd_verify_txns( fd_ed25519_amd_t * e, ulong txn_cnt, uchar const * payload, uint const * txn_off,
                            uint const * txn_sz, ulong payload_sz, schar * txn_err, uint * sig_base, schar * sig_err ) {
  return fd_ed25519_amd_verify_txns_tag( e, txn_cnt, payload, txn_off, txn_sz, payload_sz, txn_err, sig_base, sig_err, NULL, NULL );
}

extern "C" int
fd_ed25519_amd_verify_txns_tag( fd_ed25519_amd_t * e, ulong txn_cnt, uchar const * payload, uint const * txn_off,
                                uint const * txn_sz, ulong payload_sz, schar * txn_err, uint * sig_base, schar * sig_err,
                                ulong * txn_tag, ulong * sig_tag ) {
  return fd_ed25519_amd_verify_txns_budget( e, txn_cnt, payload, txn_off, txn_sz, payload_sz, txn_err, sig_base, sig_err,
                                            txn_tag, sig_tag, NULL, NULL, 0UL, NULL );
}

/* How big a descriptor can be.  A payload that parses holds at least one
   signature count byte, one 64-B signature, three header bytes, the account
   count, one 32-B account address, the 32-B blockhash and the instruction
   count: 1 + 64 + 3 + 1 + 32 + 32 + 1 = 134 bytes (a v0 payload two more).
   Behind them every instruction takes at least 3 payload bytes (program
   index and two counts) for its 10 descriptor bytes, and every lookup table
   at least 34 (address and two counts) for its 8.  With i instructions and l
   tables, 3 i + 34 l <= sz - 134, so i + 11 l <= (sz - 134)/3 rounded down,
   and the footprint 20 + 10 i + 8 l <= 20 + 10 (i + 11 l).  Up to the MTU no
   footprint exceeds FD_TXN_MAX_SZ (fd_txn.h:88-95). */
extern "C" ulong
fd_txn_amd_desc_bound( ulong payload_sz ) {
  return fd_amd_desc_bound1( payload_sz );   /* fd_ed25519_emit.h: the emit bound's host code shares it */
}
static_assert( FD_TXN_AMD_PAYLOAD_MAX == 65535UL && FD_TXN_AMD_MTU == 1232UL && FD_TXN_MAX_SZ == 3570UL,
               "fd_amd_desc_bound1 spells these out" );

/* The first buffers a transaction chunk needs on its slot. */
static int
slot_alloc_txn( fd_ed25519_amd_t const * e, slot_t * s, txn_outs_t const & o ) {
  int rc = slot_alloc_aux( s, e->cap );
  if( !rc && (o.txn_tag || o.sig_tag) ) rc = slot_alloc_tag( s, e->cap );
  if( !rc && ( o.desc_off || s->emit_arm.out ) ) rc = slot_alloc_desc( s, e->cap, e->blob_cap );   /* frames: the packed descriptors' source */
  if( !rc && o.budget ) rc = slot_alloc_budget( s, e->cap );
  return rc;
}

/* The output-argument check of every transaction call, staged (SZ = uint)
   or registered (SZ = ulong): sig_base given whenever a per-signature output
   (sig_err, sig_tag) is; desc and desc_off both or neither; and desc_cap at
   least the sum of fd_txn_amd_desc_bound (the descriptor capacity is decided
   by the bound, never by the data).  txn_sz: not NULL when txn_cnt > 0. */
template<typename SZ>
static int
txn_outs_check( ulong txn_cnt, SZ const * txn_sz, uint const * sig_base, schar const * sig_err, ulong const * sig_tag,
                ulong const * desc_off, uchar const * desc, ulong desc_cap ) {
  if( (sig_err || sig_tag) && !sig_base ) return FD_ED25519_AMD_ERR_INVAL;
  if( !desc != !desc_off ) return FD_ED25519_AMD_ERR_INVAL;
  if( desc_off ) {
    ulong need = 0;
    for( ulong t=0; t<txn_cnt; t++ ) need += fd_txn_amd_desc_bound( txn_sz[t] );
    if( desc_cap < need ) return FD_ED25519_AMD_ERR_INVAL;
  }
  return FD_ED25519_AMD_OK;
}

int
fd_amd_txn_args_check( fd_ed25519_amd_t const * e, ulong txn_cnt, uchar const * payload, uint const * txn_off,
                       uint const * txn_sz, ulong payload_sz, schar const * txn_err, uint const * sig_base,
                       schar const * sig_err, ulong const * sig_tag, ulong const * desc_off, uchar const * desc,
                       ulong desc_cap ) {
  if( !e || (txn_cnt && (!payload || !txn_off || !txn_sz || !txn_err)) ) return FD_ED25519_AMD_ERR_INVAL;
  if( txn_outs_check( txn_cnt, txn_sz, sig_base, sig_err, sig_tag, desc_off, desc, desc_cap ) ) return FD_ED25519_AMD_ERR_INVAL;
  for( ulong t=0; t<txn_cnt; t++ ) {
    if( txn_sz[t] > FD_TXN_AMD_MTU || (ulong)txn_off[t] + txn_sz[t] > payload_sz || txn_sz[t] > e->blob_cap )
      return FD_ED25519_AMD_ERR_INVAL;
    if( fd_amd_txn_slots1( payload + txn_off[t], txn_sz[t] ) > e->cap ) return FD_ED25519_AMD_ERR_INVAL;
  }
  return FD_ED25519_AMD_OK;
}

/* The chunk rule of the staged transaction calls, stated once: the chunk cut
   off the front of txn_cnt transactions is bounded by their count, their
   signature slots and their bytes.  take( j, p, sz, bsz, ns ) is called for
   every transaction j the chunk takes: its payload p of sz bytes, and the
   bytes and signature slots of the chunk before it.  A payload's first
   byte, which gives its slots, is read from caller memory once per decision:
   the read that bounds the chunk (ns <= cap is what keeps the slot's planes
   in bounds) is the one whose running sum `take` stages.  Returns the
   transactions taken, their bytes in *bytes and their slots in *slots. */
template<typename TAKE>
static ulong
txns_chunk( fd_ed25519_amd_t const * e, ulong txn_cnt, uchar const * payload, uint const * txn_off, uint const * txn_sz,
            ulong * bytes, ulong * slots, TAKE take ) {
  ulong c = 0, bsz = 0, ns = 0;
  while( c < txn_cnt && c < e->cap ) {
    uchar const * p = payload + txn_off[c];
    ulong sz = txn_sz[c], k2 = fd_amd_txn_slots1( p, sz );
    if( bsz + sz > e->blob_cap || ns + k2 > e->cap ) break;
    take( c, p, sz, bsz, ns );
    bsz += sz; ns += k2; c++;
  }
  *bytes = bsz; *slots = ns;
  return c;
}

/* Stage and launch on s the first chunk of the txn_cnt transactions given
   (txn_off and txn_sz start at the chunk's first transaction); returns the
   transactions taken or an error code, and in *slots the signature slots
   they reserve. */
static long
stage_txns( fd_ed25519_amd_t * e, slot_t * s, ulong txn_cnt, uchar const * payload, uint const * txn_off,
            uint const * txn_sz, txn_outs_t const & o, ulong * slots ) {
  int rc = slot_alloc_txn( e, s, o );
  if( rc ) return rc;
  ulong bsz = 0, bound = 0;
  ulong const c = txns_chunk( e, txn_cnt, payload, txn_off, txn_sz, &bsz, slots,
                              [&]( ulong j, uchar const * p, ulong sz, ulong b, ulong ns ) {
    if( sz ) memcpy( s->h_blob + b, p, sz );
    s->h_toff[j] = (uint32_t)b; s->h_tsz[j] = (uint32_t)sz; s->h_tbase[j] = (uint32_t)ns;
    if( o.desc_off ) bound += fd_txn_amd_desc_bound( sz );
  } );
  s->h_tbase[c] = (uint32_t)*slots;
  rc = slot_launch_txn( s, c, *slots, bsz, o, bound );
  return rc ? rc : (long)c;
}

extern "C" int
fd_ed25519_amd_verify_txns_desc( fd_ed25519_amd_t * e, ulong txn_cnt, uchar const * payload, uint const * txn_off,
                                 uint const * txn_sz, ulong payload_sz, schar * txn_err, uint * sig_base, schar * sig_err,
                                 ulong * txn_tag, ulong * sig_tag, ulong * desc_off, uchar * desc, ulong desc_cap ) {
  return fd_ed25519_amd_verify_txns_budget( e, txn_cnt, payload, txn_off, txn_sz, payload_sz, txn_err, sig_base, sig_err,
                                            txn_tag, sig_tag, desc_off, desc, desc_cap, NULL );
}

extern "C" int
fd_ed25519_amd_verify_txns_budget( fd_ed25519_amd_t * e, ulong txn_cnt, uchar const * payload, uint const * txn_off,
                                   uint const * txn_sz, ulong payload_sz, schar * txn_err, uint * sig_base, schar * sig_err,
                                   ulong * txn_tag, ulong * sig_tag, ulong * desc_off, uchar * desc, ulong desc_cap,
                                   fd_txn_amd_budget_t * budget ) {
  if( SYNC_REFUSED( e ) ) return FD_ED25519_AMD_ERR_INVAL;
  int rc = fd_amd_txn_args_check( e, txn_cnt, payload, txn_off, txn_sz, payload_sz, txn_err, sig_base, sig_err, sig_tag,
                                  desc_off, desc, desc_cap );
  if( rc ) return rc;
  if( desc_off ) desc_off[0] = 0UL;
  ulong dbase = 0;   /* descriptor bytes of the chunks delivered so far */
  /* global signature numbering (the caller-visible sig_base) */
  if( sig_base ) fd_ed25519_amd_txn_slots( txn_cnt, payload, txn_off, txn_sz, sig_base );
  ulong gsig = 0;
  return run_ring( e, 2, txn_cnt, [&]( slot_t * s, ulong t ) -> long {
    txn_outs_t o = { txn_err + t, sig_err ? sig_err + gsig : NULL, txn_tag ? txn_tag + t : NULL,
                     sig_tag ? sig_tag + gsig : NULL, desc_off ? desc_off + t : NULL, desc, desc_cap, &dbase,
                     budget ? budget + t : NULL };
    ulong ns = 0;
    long c = stage_txns( e, s, txn_cnt - t, payload, txn_off + t, txn_sz + t, o, &ns );
    gsig += ns;
    return c;
  } );
}

/* ------------------------------------------------------------------ */
/* transaction batches gathered by the GPU from registered memory       */

extern "C" ulong
fd_ed25519_amd_txn_slots_ptrs( ulong txn_cnt, void const * const * txn, ulong const * txn_sz, uint * tbase ) {
  ulong acc = 0;
  for( ulong t=0; t<txn_cnt; t++ ) {
    tbase[t] = (uint)acc;
    if( txn_sz[t] && txn[t] ) acc += fd_amd_txn_slots1( (uchar const *)txn[t], txn_sz[t] );
  }
  tbase[txn_cnt] = (uint)acc;
  return acc;
}

/* The one place that sizes a gathered transaction chunk: fd_ed25519_amd_gather_layout's
   rule with the signature slots as a third bound (every payload fits a chunk
   alone: the callers check its size and its slots up front).  dst[j]:
   payload j's offset in the chunk's blob, a multiple of 16; it owns
   [dst[j], dst[j] + round_up( sz[j], 16 )).  Pure host code. */
extern "C" ulong
fd_ed25519_amd_txn_gather_layout( ulong n, ulong const * sz, uint const * slots, ulong cap, ulong blob_cap, uint * dst,
                                  ulong * slot_cnt ) {
  ulong c = 0, b = 0, ns = 0;
  while( c < n ) {
    ulong const pad = (sz[c] + 15UL) & ~15UL;
    if( c && ( c >= cap || ns + slots[c] > cap || sz[c] > blob_cap || b + pad > blob_cap ) ) break;
    dst[c] = (uint)b;
    b += pad; ns += slots[c]; c++;
  }
  *slot_cnt = ns;
  return c;
}

/* Chunk of c transactions whose records sit in s->h_pack: k_gather_txn
   fetches the payloads into d_blob and writes d_toff, d_tsz and
   d_tbase[0..c] (d_tbase[c] = nslot), then the kernels of slot_launch_txn --
   without its four host-to-device copies: the records reach the kernel in
   place (it reads the mapped h_pack, 32 B per transaction, once), as
   slot_launch_gather's do. */
static int
slot_launch_txn_gather( slot_t * s, ulong c, ulong nslot, uint waves, txn_outs_t const & o, ulong desc_bound ) {
  /* A throughput chunk's gather runs beside the other slots' verify kernels
     and its reads of host memory hold up their memory traffic
     (slot_launch_gather): capped at `waves` waves, 64 unless
     FD_ED25519_AMD_GATHER_TXN_WAVES says otherwise (32 / 64 / 128 measured:
     profiles/txns_registered_cost.json).  A chunk small enough for the
     latency kernels is a batch of its own with nothing beside it: no cap. */
  bool const lat = fd_amd_uses_latency_path( (uint32_t)nslot, 0 ) != 0;
  if( fd_amd_launch_gather_txn( (uint32_t)c, (fd_amd_gather_txn_rec_t const *)s->m_pack, s->d_blob, s->d_toff, s->d_tsz,
                                s->d_tbase, (uint32_t)nslot, lat ? 0u : waves, s->stream ) )
    return FD_ED25519_AMD_ERR_DEVICE;
  return slot_launch_txn_dev( s, c, nslot, o, desc_bound );
}

extern "C" int
fd_ed25519_amd_verify_txns_registered( fd_ed25519_amd_t * e, ulong txn_cnt, void const * const * txn, ulong const * txn_sz,
                                       schar * txn_err, uint * sig_base, schar * sig_err ) {
  return fd_ed25519_amd_verify_txns_registered_tag( e, txn_cnt, txn, txn_sz, txn_err, sig_base, sig_err, NULL, NULL );
}

extern "C" int
fd_ed25519_amd_verify_txns_registered_tag( fd_ed25519_amd_t * e, ulong txn_cnt, void const * const * txn,
                                           ulong const * txn_sz, schar * txn_err, uint * sig_base, schar * sig_err,
                                           ulong * txn_tag, ulong * sig_tag ) {
  return fd_ed25519_amd_verify_txns_registered_budget( e, txn_cnt, txn, txn_sz, txn_err, sig_base, sig_err, txn_tag, sig_tag,
                                                       NULL, NULL, 0UL, NULL );
}

/* The argument check of the registered transaction calls, after e and the
   count: the arrays and the outputs (txn_outs_check), then every transaction
   before anything launches: its pointer, its size, its first and last byte
   in one registration of the table (16 B of pointer and size read per
   transaction), and the signature slots it reserves -- read here, once,
   from payload[0] into slots[0 .. txn_cnt): the chunks and sig_base use this
   count, whatever the byte holds later. */
static int
txns_registered_check( fd_ed25519_amd_t const * e, reg_view_t const & view, ulong txn_cnt, void const * const * txn,
                       ulong const * txn_sz, schar const * txn_err, uint const * sig_base, schar const * sig_err,
                       ulong const * sig_tag, ulong const * desc_off, uchar const * desc, ulong desc_cap, uint * slots ) {
  if( txn_cnt && (!txn || !txn_sz || !txn_err) ) return FD_ED25519_AMD_ERR_INVAL;
  if( txn_outs_check( txn_cnt, txn_sz, sig_base, sig_err, sig_tag, desc_off, desc, desc_cap ) ) return FD_ED25519_AMD_ERR_INVAL;
  bool const ok = check_par( txn_cnt, [&]( ulong lo, ulong hi ) -> bool {
    reg_view_t v = view;                     /* its own last-hit index */
    for( ulong t=lo; t<hi; t++ ) {
      ulong const sz = txn_sz[t];
      uint64_t dev;
      if( !sz ) { slots[t] = 0U; continue; }
      if( sz > FD_TXN_AMD_MTU || sz > e->blob_cap || !txn[t] || !v.xlat( txn[t], sz, &dev ) ) return false;
      ulong const k = fd_amd_txn_slots1( (uchar const *)txn[t], sz );
      if( k > e->cap ) return false;
      slots[t] = (uint)k;
    }
    return true;
  } );
  return ok ? FD_ED25519_AMD_OK : FD_ED25519_AMD_ERR_INVAL;
}

/* The caller-visible global signature numbering from the checked counts. */
static void
txns_sig_base( ulong txn_cnt, uint const * slots, uint * sig_base ) {
  ulong acc = 0;
  for( ulong t=0; t<txn_cnt; t++ ) { sig_base[t] = (uint)acc; acc += slots[t]; }
  sig_base[txn_cnt] = (uint)acc;
}

/* Stage and launch on s the first chunk of the txn_cnt registered
   transactions given (txn, txn_sz and slots start at the chunk's first
   transaction); returns the transactions taken or an error code, and in
   *slot_cnt the signature slots they reserve. */
static long
stage_txns_registered( fd_ed25519_amd_t * e, slot_t * s, reg_view_t & view, ulong txn_cnt, void const * const * txn,
                       ulong const * txn_sz, uint const * slots, txn_outs_t const & o, ulong * slot_cnt ) {
  int rc = slot_alloc_txn( e, s, o );
  if( rc ) return rc;
  /* the chunk's records in h_pack (32 B per transaction), their dst behind them */
  fd_amd_gather_txn_rec_t * rec = (fd_amd_gather_txn_rec_t *)s->h_pack;
  uint * dst = slot_gather_dst( e, s );
  ulong ns = 0;
  ulong c = fd_ed25519_amd_txn_gather_layout( txn_cnt, txn_sz, slots, e->cap, e->blob_cap, dst, &ns );
  ulong b = 0, bound = 0;
  for( ulong j=0; j<c; j++ ) {
    /* translated again, not kept from the check (fd_ed25519_amd_verify_batch_registered):
       an address the table does not give never reaches the kernel */
    ulong const sz = txn_sz[j];
    rec[j].src = 0UL;
    if( sz > FD_TXN_AMD_MTU || sz > e->blob_cap || ( sz && ( !txn[j] || !view.xlat( txn[j], sz, &rec[j].src ) ) ) )
      return FD_ED25519_AMD_ERR_INVAL;
    rec[j].sz = (uint32_t)sz; rec[j].dst = dst[j]; rec[j].tbase = (uint32_t)b;
    if( o.desc_off ) bound += fd_txn_amd_desc_bound( sz );
    b += slots[j];
  }
  rc = slot_launch_txn_gather( s, c, ns, (uint)e->gather_txn_waves, o, bound );
  *slot_cnt = ns;
  return rc ? rc : (long)c;
}

extern "C" int
fd_ed25519_amd_verify_txns_registered_desc( fd_ed25519_amd_t * e, ulong txn_cnt, void const * const * txn,
                                            ulong const * txn_sz, schar * txn_err, uint * sig_base, schar * sig_err,
                                            ulong * txn_tag, ulong * sig_tag, ulong * desc_off, uchar * desc,
                                            ulong desc_cap ) {
  return fd_ed25519_amd_verify_txns_registered_budget( e, txn_cnt, txn, txn_sz, txn_err, sig_base, sig_err, txn_tag, sig_tag,
                                                       desc_off, desc, desc_cap, NULL );
}

extern "C" int
fd_ed25519_amd_verify_txns_registered_budget( fd_ed25519_amd_t * e, ulong txn_cnt, void const * const * txn,
                                              ulong const * txn_sz, schar * txn_err, uint * sig_base, schar * sig_err,
                                              ulong * txn_tag, ulong * sig_tag, ulong * desc_off, uchar * desc,
                                              ulong desc_cap, fd_txn_amd_budget_t * budget ) {
  if( SYNC_REFUSED( e ) || !e || txn_cnt > 0xFFFFFFFFUL ) return FD_ED25519_AMD_ERR_INVAL;
  reg_view_t view;
  std::vector<uint> slots( txn_cnt );
  int rc = txns_registered_check( e, view, txn_cnt, txn, txn_sz, txn_err, sig_base, sig_err, sig_tag, desc_off, desc,
                                  desc_cap, slots.data() );
  if( rc ) return rc;
  if( desc_off ) desc_off[0] = 0UL;
  if( sig_base ) txns_sig_base( txn_cnt, slots.data(), sig_base );
  if( !txn_cnt ) return FD_ED25519_AMD_OK;   /* before anything touches the device */
  ulong gsig = 0;
  ulong dbase = 0;   /* descriptor bytes of the chunks delivered so far */
  return run_ring( e, e->nslot, txn_cnt, [&]( slot_t * s, ulong t ) -> long {
    txn_outs_t o = { txn_err + t, sig_err ? sig_err + gsig : NULL, txn_tag ? txn_tag + t : NULL,
                     sig_tag ? sig_tag + gsig : NULL, desc_off ? desc_off + t : NULL, desc, desc_cap, &dbase,
                     budget ? budget + t : NULL };
    ulong ns = 0;
    long c = stage_txns_registered( e, s, view, txn_cnt - t, txn + t, txn_sz + t, slots.data() + t, o, &ns );
    gsig += ns;
    return c;
  } );
}

/* Device-resident transaction batch: workspace = verify workspace for
   slot_cnt signatures + the signature layout planes + footprints. */
namespace {
struct txn_ws_t { size_t vws, pub, sig, off, sz, skip, err, fp, total; };
inline size_t al256( size_t x ) { return (x + 255UL) & ~(size_t)255UL; }
txn_ws_t txn_ws_layout( ulong txn_cnt, ulong slot_cnt ) {
  txn_ws_t L; size_t o = 0; ulong S = slot_cnt ? slot_cnt : 1UL;
  L.vws  = o; o = al256( o + fd_amd_ws_layout( S ).total );
  L.pub  = o; o = al256( o + 32UL*S );
  L.sig  = o; o = al256( o + 64UL*S );
  L.off  = o; o = al256( o + 4UL*S );
  L.sz   = o; o = al256( o + 4UL*S );
  L.skip = o; o = al256( o + S );
  L.err  = o; o = al256( o + S );
  L.fp   = o; o = al256( o + 4UL*(txn_cnt ? txn_cnt : 1UL) );
  L.total = o;
  return L;
}
}

extern "C" ulong
fd_ed25519_amd_txn_workspace_footprint( ulong txn_cnt, ulong slot_cnt ) {
  return txn_ws_layout( txn_cnt, slot_cnt ).total;
}

extern "C" ulong
fd_ed25519_amd_txn_slots( ulong txn_cnt, uchar const * payload, uint const * txn_off, uint const * txn_sz,
                          uint * tbase ) {
  ulong acc = 0;
  for( ulong t=0; t<txn_cnt; t++ ) { tbase[t] = (uint)acc; acc += fd_amd_txn_slots1( payload + txn_off[t], txn_sz[t] ); }
  tbase[txn_cnt] = (uint)acc;
  return acc;
}

extern "C" int
fd_ed25519_amd_verify_txns_dev( ulong txn_cnt, ulong slot_cnt, uchar const * d_payload, uint const * d_txn_off,
                                uint const * d_txn_sz, uint const * d_tbase, schar * d_txn_err, schar * d_sig_err,
                                void * d_ws, void * stream ) {
  return fd_ed25519_amd_verify_txns_dev_mode( txn_cnt, slot_cnt, d_payload, d_txn_off, d_txn_sz, d_tbase, d_txn_err,
                                              d_sig_err, d_ws, stream, FD_ED25519_AMD_MODE_REFERENCE );
}

extern "C" int
fd_ed25519_amd_verify_txns_dev_mode( ulong txn_cnt, ulong slot_cnt, uchar const * d_payload, uint const * d_txn_off,
                                     uint const * d_txn_sz, uint const * d_tbase, schar * d_txn_err, schar * d_sig_err,
                                     void * d_ws, void * stream, int mode ) {
  if( !fd_amd_mode_ok( mode ) ) return FD_ED25519_AMD_ERR_INVAL;
  if( txn_cnt > 0xFFFFFFFFUL || slot_cnt > 0xFFFFFFFFUL ) return FD_ED25519_AMD_ERR_INVAL;
  if( !txn_cnt ) return FD_ED25519_AMD_OK;
  if( !d_payload || !d_txn_off || !d_txn_sz || !d_tbase || !d_txn_err || !d_ws ) return FD_ED25519_AMD_ERR_INVAL;
  txn_ws_t L = txn_ws_layout( txn_cnt, slot_cnt );
  uint8_t * w = (uint8_t *)d_ws;
  hipStream_t st = (hipStream_t)stream;
  int8_t * err = d_sig_err ? (int8_t *)d_sig_err : (int8_t *)(w + L.err);
  if( fd_amd_launch_txn_parse( (uint32_t)txn_cnt, d_payload, d_txn_off, d_txn_sz, (uint32_t *)(w + L.fp), NULL, 0,
                               d_tbase, w + L.pub, w + L.sig, (uint32_t *)(w + L.off), (uint32_t *)(w + L.sz),
                               (int8_t *)(w + L.skip), st ) )
    return FD_ED25519_AMD_ERR_DEVICE;
  if( slot_cnt && fd_amd_launch_verify( (uint32_t)slot_cnt, w + L.pub, w + L.sig, (uint32_t *)(w + L.off),
                                        (uint32_t *)(w + L.sz), d_payload, err, w + L.vws, st, 1, NULL,
                                        (int8_t *)(w + L.skip), 0, NULL, mode == FD_ED25519_AMD_MODE_STRICT ) )
    return FD_ED25519_AMD_ERR_DEVICE;
  /* k_txn_reduce after k_strict, on the same stream */
  if( fd_amd_launch_txn_reduce( (uint32_t)txn_cnt, (uint32_t *)(w + L.fp), d_tbase, err, (int8_t *)d_txn_err, st ) )
    return FD_ED25519_AMD_ERR_DEVICE;
  return FD_ED25519_AMD_OK;
}

extern "C" int
fd_txn_amd_parse_dev( ulong txn_cnt, uchar const * d_payload, uint const * d_txn_off, uint const * d_txn_sz,
                      uint * d_footprint, uchar * d_out, ulong out_stride, void * stream ) {
  if( txn_cnt > 0xFFFFFFFFUL ) return FD_ED25519_AMD_ERR_INVAL;
  if( !txn_cnt ) return FD_ED25519_AMD_OK;
  if( !d_payload || !d_txn_off || !d_txn_sz || !d_footprint ) return FD_ED25519_AMD_ERR_INVAL;
  if( d_out && (out_stride < FD_TXN_MAX_SZ || (out_stride & 1UL)) ) return FD_ED25519_AMD_ERR_INVAL;
  if( fd_amd_launch_txn_parse( (uint32_t)txn_cnt, d_payload, d_txn_off, d_txn_sz, d_footprint, d_out, out_stride,
                               NULL, NULL, NULL, NULL, NULL, NULL, (hipStream_t)stream ) )
    return FD_ED25519_AMD_ERR_DEVICE;
  return FD_ED25519_AMD_OK;
}

extern "C" int
fd_txn_amd_budget_dev( ulong txn_cnt, uchar const * d_payload, uint const * d_txn_off, uint const * d_txn_sz,
                       uint const * d_footprint, fd_txn_amd_budget_t * d_budget, void * stream ) {
  if( txn_cnt > 0xFFFFFFFFUL ) return FD_ED25519_AMD_ERR_INVAL;
  if( !txn_cnt ) return FD_ED25519_AMD_OK;
  if( !d_payload || !d_txn_off || !d_txn_sz || !d_footprint || !d_budget || ( (ulong)d_budget & 7UL ) ) return FD_ED25519_AMD_ERR_INVAL;
  if( fd_amd_launch_txn_budget( (uint32_t)txn_cnt, d_payload, d_txn_off, d_txn_sz, d_footprint, d_budget, (hipStream_t)stream ) )
    return FD_ED25519_AMD_ERR_DEVICE;
  return FD_ED25519_AMD_OK;
}

extern "C" ulong
fd_txn_amd_parse_packed_scratch_footprint( ulong txn_cnt ) {
  ulong nblk = ( txn_cnt + 63UL )/64UL;   /* one 64-bit total per 64 transactions */
  return al256( 8UL*( nblk ? nblk : 1UL ) );
}

extern "C" int
fd_txn_amd_parse_packed_dev( ulong txn_cnt, uchar const * d_payload, uint const * d_txn_off, uint const * d_txn_sz,
                             uint * d_footprint, ulong * d_desc_off, uchar * d_desc, ulong desc_cap, void * d_scratch,
                             void * stream ) {
  if( txn_cnt > 0xFFFFFFFFUL || !d_desc_off ) return FD_ED25519_AMD_ERR_INVAL;
  if( txn_cnt && ( !d_payload || !d_txn_off || !d_txn_sz || !d_footprint || !d_scratch ) ) return FD_ED25519_AMD_ERR_INVAL;
  if( ( desc_cap && !d_desc ) || ( (ulong)d_desc & 1UL ) || ( (ulong)d_desc_off & 7UL ) || ( (ulong)d_scratch & 7UL ) )
    return FD_ED25519_AMD_ERR_INVAL;
  /* footprint pass: the validate-only parse; then the scan and the store pass */
  if( fd_amd_launch_txn_parse( (uint32_t)txn_cnt, d_payload, d_txn_off, d_txn_sz, d_footprint, NULL, 0, NULL, NULL, NULL,
                               NULL, NULL, NULL, (hipStream_t)stream ) ||
      fd_amd_launch_txn_pack( (uint32_t)txn_cnt, d_payload, d_txn_off, d_txn_sz, d_footprint, (uint64_t *)d_scratch,
                              (uint64_t *)d_desc_off, d_desc, desc_cap, (hipStream_t)stream ) )
    return FD_ED25519_AMD_ERR_DEVICE;
  return FD_ED25519_AMD_OK;
}

extern "C" int
fd_ed25519_amd_sign_dev( ulong n, uchar const * d_prv, uint const * d_msg_off, uint const * d_msg_sz,
                         uchar const * d_blob, uchar * d_pub, uchar * d_sig, void * stream ) {
  if( n > 0xFFFFFFFFUL ) return FD_ED25519_AMD_ERR_INVAL;
  if( !n ) return FD_ED25519_AMD_OK;
  if( !d_prv || !d_msg_off || !d_msg_sz || !d_blob || !d_pub || !d_sig ) return FD_ED25519_AMD_ERR_INVAL;
  if( fd_amd_launch_sign( (uint32_t)n, d_prv, d_msg_off, d_msg_sz, d_blob, d_pub, d_sig, (hipStream_t)stream ) )
    return FD_ED25519_AMD_ERR_DEVICE;
  return FD_ED25519_AMD_OK;
}

extern "C" ulong
fd_ed25519_amd_workspace_footprint( ulong n ) {
  return fd_amd_ws_layout( n ).total;
}

/* Host only: the layout the kernels are launched with, for tests that
   look at (or fill) single planes of a workspace. */
extern "C" void
fd_ed25519_amd_debug_ws_layout( ulong n, ulong * out ) {
  if( !out ) return;
  ws_layout_t L = fd_amd_ws_layout( n );
  size_t const v[ FD_ED25519_AMD_WS_LAYOUT_CNT ] = { L.N, L.dig, L.evn, L.top, L.A, L.R, L.Ai, L.st, L.tag, L.ds, L.init,
                                                     L.ctr, L.total };
  for( int k=0; k<FD_ED25519_AMD_WS_LAYOUT_CNT; k++ ) out[k] = (ulong)v[k];
}

extern "C" int
fd_ed25519_amd_verify_dev_ev_mode( ulong n, uchar const * d_pub, uchar const * d_sig, uint const * d_msg_off,
                                   uint const * d_msg_sz, uchar const * d_blob, schar * d_err, void * d_ws,
                                   void * stream, void * const * ev, int mode ) {
  if( !fd_amd_mode_ok( mode ) ) return FD_ED25519_AMD_ERR_INVAL;   /* before anything touches a device */
  if( n > 0xFFFFFFFFUL ) return FD_ED25519_AMD_ERR_INVAL;
  if( !n ) return FD_ED25519_AMD_OK;
  if( !d_pub || !d_sig || !d_msg_off || !d_msg_sz || !d_blob || !d_err || !d_ws ) return FD_ED25519_AMD_ERR_INVAL;
  if( fd_amd_launch_verify( (uint32_t)n, d_pub, d_sig, d_msg_off, d_msg_sz, d_blob, (int8_t *)d_err, d_ws,
                            (hipStream_t)stream, 1, (hipEvent_t const *)ev, NULL, 0, NULL,
                            mode == FD_ED25519_AMD_MODE_STRICT ) )
    return FD_ED25519_AMD_ERR_DEVICE;
  return FD_ED25519_AMD_OK;
}

extern "C" int
fd_ed25519_amd_verify_dev_mode( ulong n, uchar const * d_pub, uchar const * d_sig, uint const * d_msg_off,
                                uint const * d_msg_sz, uchar const * d_blob, schar * d_err, void * d_ws, void * stream,
                                int mode ) {
  return fd_ed25519_amd_verify_dev_ev_mode( n, d_pub, d_sig, d_msg_off, d_msg_sz, d_blob, d_err, d_ws, stream, NULL, mode );
}

extern "C" int
fd_ed25519_amd_verify_dev( ulong n, uchar const * d_pub, uchar const * d_sig, uint const * d_msg_off,
                           uint const * d_msg_sz, uchar const * d_blob, schar * d_err, void * d_ws, void * stream ) {
  return fd_ed25519_amd_verify_dev_ev_mode( n, d_pub, d_sig, d_msg_off, d_msg_sz, d_blob, d_err, d_ws, stream, NULL,
                                            FD_ED25519_AMD_MODE_REFERENCE );
}

extern "C" int
fd_ed25519_amd_verify_dev_ev( ulong n, uchar const * d_pub, uchar const * d_sig, uint const * d_msg_off,
                              uint const * d_msg_sz, uchar const * d_blob, schar * d_err, void * d_ws, void * stream,
                              void * const * ev ) {
  return fd_ed25519_amd_verify_dev_ev_mode( n, d_pub, d_sig, d_msg_off, d_msg_sz, d_blob, d_err, d_ws, stream, ev,
                                            FD_ED25519_AMD_MODE_REFERENCE );
}

/* ------------------------------------------------------------------ */
/* asynchronous submissions: one chunk on one slot, collected later     */

extern "C" ulong
fd_ed25519_amd_async_depth( fd_ed25519_amd_t const * e ) { return e ? (ulong)e->nslot : 0UL; }

extern "C" ulong
fd_ed25519_amd_async_in_flight( fd_ed25519_amd_t const * e ) { return e ? (ulong)e->a_cnt : 0UL; }

/* The slot the next submission takes, after the submit call's argument
   checks: NULL with *rc set when every slot carries one, or the device
   cannot be made current. */
static slot_t *
submit_slot( fd_ed25519_amd_t * e, int * rc ) {
  if( e->a_cnt >= e->nslot ) { *rc = FD_ED25519_AMD_ERR_BUSY; return NULL; }
  if( hipSetDevice( e->device ) != hipSuccess ) { *rc = FD_ED25519_AMD_ERR_DEVICE; return NULL; }
  return &e->slot[e->a_tail];
}

/* Run a stage function once on s as the next submission.  The ticket is
   handed out only when the chunk is in flight.  ERR_INVAL from the stage comes
   before its first launch; any other error quiesces the engine, as in
   run_ring.  keep / keep_cnt (both or neither: KEEP_ARGS_BAD): a _keep
   submission, whose launch tail adds the survivor filter; the slot's buffers
   for it are allocated here, on first use. */
#define KEEP_ARGS_BAD( keep, keep_cnt ) ( !(keep) != !(keep_cnt) )

/* The emit arguments of an _emit submission, before anything else happens:
   all four or none (none: em->out stays NULL and the call is the _keep one);
   with keep; out 64-aligned; [out, out + out_cap) inside ONE registration of
   fd_ed25519_amd_host_register's table, the only source of the address the
   store kernel gets.  The capacity is checked by the callers against the sum
   of the bound (emit_cap_ok), never against the data. */
static int
emit_args_check( emit_args_t * em, void * out, ulong out_cap, ulong * emit_off, uint * emit_sz, uint const * keep ) {
  *em = emit_args_t{ NULL, 0UL, NULL, NULL, 0UL };
  if( !out && !out_cap && !emit_off && !emit_sz ) return FD_ED25519_AMD_OK;
  if( !out || !out_cap || !emit_off || !emit_sz || !keep || ( (uintptr_t)out & 63UL ) ) return FD_ED25519_AMD_ERR_INVAL;
  reg_view_t view;
  uint64_t dev;
  if( !view.xlat( out, out_cap, &dev ) ) return FD_ED25519_AMD_ERR_INVAL;
  *em = emit_args_t{ out, out_cap, emit_off, emit_sz, dev };
  return FD_ED25519_AMD_OK;
}

template<typename SZ>
static bool
emit_cap_ok( emit_args_t const & em, ulong n, SZ const * sz, bool txn ) {
  if( !em.out ) return true;
  ulong need = 0UL;
  for( ulong i=0; i<n; i++ ) need += txn ? fd_txn_amd_emit_bound( (ulong)sz[i] ) : fd_ed25519_amd_emit_bound( (ulong)sz[i] );
  return em.cap >= need;
}

template<typename STAGE>
static int
submit_run( fd_ed25519_amd_t * e, slot_t * s, uint * keep, ulong * keep_cnt, emit_args_t const & em, ulong * ticket, STAGE stage ) {
  if( keep ) { int rc = slot_alloc_keep( s, e->cap ); if( rc ) return engine_quiesce( e, rc ); }
  if( em.out ) { int rc = slot_alloc_emit( s, e->cap ); if( rc ) return engine_quiesce( e, rc ); }
  s->ticket = e->ticket + 1UL;
  s->tick_arm = !e->poll_event;
  s->keep_arm = keep; s->kcnt_arm = keep_cnt; s->win_arm = keep ? e->win : NULL;
  s->emit_arm = em;
  long c = stage();
  s->tick_arm = 0;
  s->keep_arm = NULL; s->kcnt_arm = NULL; s->win_arm = NULL;
  s->emit_arm.out = NULL;
  if( c < 0L ) return c == (long)FD_ED25519_AMD_ERR_INVAL ? FD_ED25519_AMD_ERR_INVAL : engine_quiesce( e, (int)c );
  e->ticket = s->ticket;
  e->a_tail = (e->a_tail + 1) % e->nslot; e->a_cnt++;
  *ticket = s->ticket;
  return FD_ED25519_AMD_OK;
}

extern "C" int
fd_ed25519_amd_submit_batch( fd_ed25519_amd_t * e, ulong n, void const * const * msg, ulong const * sz,
                             void const * const * sig, void const * const * pub, schar * err, ulong * tag, ulong * ticket ) {
  return fd_ed25519_amd_submit_batch_keep( e, n, msg, sz, sig, pub, err, tag, NULL, NULL, ticket );
}

extern "C" int
fd_ed25519_amd_submit_batch_keep( fd_ed25519_amd_t * e, ulong n, void const * const * msg, ulong const * sz,
                                  void const * const * sig, void const * const * pub, schar * err, ulong * tag,
                                  uint * keep, ulong * keep_cnt, ulong * ticket ) {
  return fd_ed25519_amd_submit_batch_emit( e, n, msg, sz, sig, pub, err, tag, keep, keep_cnt, NULL, 0UL, NULL, NULL, ticket );
}

extern "C" int
fd_ed25519_amd_submit_batch_emit( fd_ed25519_amd_t * e, ulong n, void const * const * msg, ulong const * sz,
                                  void const * const * sig, void const * const * pub, schar * err, ulong * tag,
                                  uint * keep, ulong * keep_cnt, void * out, ulong out_cap, ulong * emit_off, uint * emit_sz,
                                  ulong * ticket ) {
  if( !e || !ticket || !n || KEEP_ARGS_BAD( keep, keep_cnt ) ) return FD_ED25519_AMD_ERR_INVAL;
  emit_args_t em;
  if( emit_args_check( &em, out, out_cap, emit_off, emit_sz, keep ) ) return FD_ED25519_AMD_ERR_INVAL;
  int rc = batch_args_check( e, n, msg, sz, sig, pub, err );
  if( rc ) return rc;
  if( !emit_cap_ok( em, n, sz, false ) ) return FD_ED25519_AMD_ERR_INVAL;
  slot_t * s = submit_slot( e, &rc );
  if( !s ) return rc;
  if( batch_chunk( e, n, sz ) != n ) return FD_ED25519_AMD_ERR_INVAL;   /* one chunk */
  return submit_run( e, s, keep, keep_cnt, em, ticket, [&]() -> long { return stage_batch( e, s, n, msg, sz, sig, pub, err, tag ); } );
}

extern "C" int
fd_ed25519_amd_submit_batch_registered( fd_ed25519_amd_t * e, ulong n, void const * const * msg, ulong const * sz,
                                        void const * const * sig, void const * const * pub, schar * err, ulong * tag,
                                        ulong * ticket ) {
  return fd_ed25519_amd_submit_batch_registered_keep( e, n, msg, sz, sig, pub, err, tag, NULL, NULL, ticket );
}

extern "C" int
fd_ed25519_amd_submit_batch_registered_keep( fd_ed25519_amd_t * e, ulong n, void const * const * msg, ulong const * sz,
                                             void const * const * sig, void const * const * pub, schar * err, ulong * tag,
                                             uint * keep, ulong * keep_cnt, ulong * ticket ) {
  return fd_ed25519_amd_submit_batch_registered_emit( e, n, msg, sz, sig, pub, err, tag, keep, keep_cnt, NULL, 0UL, NULL, NULL,
                                                      ticket );
}

extern "C" int
fd_ed25519_amd_submit_batch_registered_emit( fd_ed25519_amd_t * e, ulong n, void const * const * msg, ulong const * sz,
                                             void const * const * sig, void const * const * pub, schar * err, ulong * tag,
                                             uint * keep, ulong * keep_cnt, void * out, ulong out_cap, ulong * emit_off,
                                             uint * emit_sz, ulong * ticket ) {
  if( !e || !ticket || !n || !msg || !sz || !sig || !pub || !err || KEEP_ARGS_BAD( keep, keep_cnt ) ) return FD_ED25519_AMD_ERR_INVAL;
  emit_args_t em;
  if( emit_args_check( &em, out, out_cap, emit_off, emit_sz, keep ) ) return FD_ED25519_AMD_ERR_INVAL;
  reg_view_t view;
  if( !batch_registered_check( e, view, n, msg, sz, sig, pub ) ) return FD_ED25519_AMD_ERR_INVAL;
  if( !emit_cap_ok( em, n, sz, false ) ) return FD_ED25519_AMD_ERR_INVAL;
  int rc;
  slot_t * s = submit_slot( e, &rc );
  if( !s ) return rc;
  /* one chunk: the layout over the whole submission, into the free slot's scratch */
  if( n > e->cap || fd_ed25519_amd_gather_layout( n, sz, e->cap, e->blob_cap, slot_gather_dst( e, s ) ) != n )
    return FD_ED25519_AMD_ERR_INVAL;
  return submit_run( e, s, keep, keep_cnt, em, ticket, [&]() -> long { return stage_batch_registered( e, s, view, n, msg, sz, sig, pub, err, tag ); } );
}

/* A frag source as the device sees it, after the submit call's checks. */
struct frag_args_t { uint64_t mcache, chunk0; ulong depth, data_sz, frag_max, seq0; };

/* What fd_ed25519_amd_submit_frags and the two _dev steps refuse about a
   source and a count, all of it O(1): true when ( src, n ) may be launched
   with dst = i * round_up( frag_max - 96, 16 ) below `blob`. */
static bool
frag_src_ok( fd_ed25519_amd_frag_src_t const * src, ulong n, ulong blob ) {
  if( !src || !src->mcache || ( (uintptr_t)src->mcache & 31UL ) || !src->chunk0 || !src->data_sz ) return false;
  if( !src->depth || ( src->depth & ( src->depth - 1UL ) ) || src->depth > ( 1UL << 40 ) || n > src->depth ) return false;
  if( src->frag_max < 96UL || src->frag_max > 65535UL ) return false;
  return n <= 0xFFFFFFFFUL && n * ( ( src->frag_max - 96UL + 15UL ) & ~15UL ) <= blob;
}

/* Stage and launch on s the n frags of a checked source: k_frag_list writes
   the records into the slot's device d_pack and the statuses into d_fstat,
   the unchanged k_gather runs on those records, and slot_launch_sig's tail
   carries k_frag_verdict (frag_arm).  The host touches no line and no frag. */
static long
stage_frags( fd_ed25519_amd_t * e, slot_t * s, frag_args_t const & fa, ulong n, schar * err, ulong * tag ) {
  int rc = slot_alloc_frags( s, e->cap );
  if( rc ) return rc;
  if( tag ) { rc = slot_alloc_tag( s, e->cap ); if( rc ) return rc; }
  fd_amd_gather_rec_t * rec = (fd_amd_gather_rec_t *)s->d_pack;
  if( fd_amd_launch_frag_list( (uint32_t)n, (void const *)fa.mcache, fa.depth, fa.seq0, fa.chunk0, fa.data_sz, (uint32_t)fa.frag_max,
                               (uint64_t)(uintptr_t)s->d_fpack, rec, s->d_fstat, s->stream ) )
    return FD_ED25519_AMD_ERR_DEVICE;
  /* the wave cap: slot_launch_gather's */
  bool const lat = fd_amd_uses_latency_path( (uint32_t)n, 0 ) != 0;
  if( fd_amd_launch_gather( (uint32_t)n, rec, s->d_pub, s->d_sig, s->d_off, s->d_sz, s->d_blob, lat ? 0u : 64u, s->stream ) )
    return FD_ED25519_AMD_ERR_DEVICE;
  s->frag_arm = { (void const *)fa.mcache, fa.depth, fa.seq0 };
  rc = slot_launch_sig( s, n, slot_planes( s ), err, tag );
  s->frag_arm = { NULL, 0UL, 0UL };
  return rc ? rc : (long)n;
}

extern "C" int
fd_ed25519_amd_submit_frags( fd_ed25519_amd_t * e, fd_ed25519_amd_frag_src_t const * src, ulong seq0, ulong n, schar * err,
                             ulong * tag, uint * keep, ulong * keep_cnt, void * out, ulong out_cap, ulong * emit_off,
                             uint * emit_sz, ulong * ticket ) {
  if( !e || !ticket || !n || !src || !err || KEEP_ARGS_BAD( keep, keep_cnt ) ) return FD_ED25519_AMD_ERR_INVAL;
  emit_args_t em;
  if( emit_args_check( &em, out, out_cap, emit_off, emit_sz, keep ) ) return FD_ED25519_AMD_ERR_INVAL;
  if( n > e->cap || !frag_src_ok( src, n, e->blob_cap ) ) return FD_ED25519_AMD_ERR_INVAL;
  /* every capacity by the bound, never by the data */
  if( em.out && em.cap < n * fd_ed25519_amd_emit_bound( src->frag_max - 96UL ) ) return FD_ED25519_AMD_ERR_INVAL;
  reg_view_t view;
  frag_args_t fa = { 0UL, 0UL, src->depth, src->data_sz, src->frag_max, seq0 };
  if( !view.xlat( src->mcache, 32UL*src->depth, &fa.mcache ) || !view.xlat( src->chunk0, src->data_sz, &fa.chunk0 ) )
    return FD_ED25519_AMD_ERR_INVAL;
  int rc;
  slot_t * s = submit_slot( e, &rc );
  if( !s ) return rc;
  return submit_run( e, s, keep, keep_cnt, em, ticket, [&]() -> long { return stage_frags( e, s, fa, n, err, tag ); } );
}

extern "C" int
fd_ed25519_amd_frag_list_dev( fd_ed25519_amd_frag_src_t const * src, ulong seq0, ulong n, void const * d_idle, void * d_rec,
                              schar * d_status, void * stream ) {
  if( !n ) return FD_ED25519_AMD_OK;
  if( !frag_src_ok( src, n, 0xFFFFFFFFUL ) || !d_idle || ( (uintptr_t)d_idle & 15UL ) || !d_rec || ( (uintptr_t)d_rec & 31UL ) ||
      !d_status )
    return FD_ED25519_AMD_ERR_INVAL;
  if( fd_amd_launch_frag_list( (uint32_t)n, src->mcache, src->depth, seq0, (uint64_t)(uintptr_t)src->chunk0, src->data_sz,
                               (uint32_t)src->frag_max, (uint64_t)(uintptr_t)d_idle, (fd_amd_gather_rec_t *)d_rec,
                               (int8_t *)d_status, (hipStream_t)stream ) )
    return FD_ED25519_AMD_ERR_DEVICE;
  return FD_ED25519_AMD_OK;
}

extern "C" int
fd_ed25519_amd_frag_check_dev( fd_ed25519_amd_frag_src_t const * src, ulong seq0, ulong n, schar * d_status, void * stream ) {
  if( !n ) return FD_ED25519_AMD_OK;
  if( !frag_src_ok( src, n, 0xFFFFFFFFUL ) || !d_status ) return FD_ED25519_AMD_ERR_INVAL;
  if( fd_amd_launch_frag_check( (uint32_t)n, src->mcache, src->depth, seq0, (int8_t *)d_status, (hipStream_t)stream ) )
    return FD_ED25519_AMD_ERR_DEVICE;
  return FD_ED25519_AMD_OK;
}

extern "C" int
fd_ed25519_amd_submit_txns( fd_ed25519_amd_t * e, ulong txn_cnt, uchar const * payload, uint const * txn_off,
                            uint const * txn_sz, ulong payload_sz, schar * txn_err, uint * sig_base, schar * sig_err,
                            ulong * txn_tag, ulong * sig_tag, ulong * desc_off, uchar * desc, ulong desc_cap,
                            ulong * ticket ) {
  return fd_ed25519_amd_submit_txns_keep( e, txn_cnt, payload, txn_off, txn_sz, payload_sz, txn_err, sig_base, sig_err, txn_tag,
                                          sig_tag, desc_off, desc, desc_cap, NULL, NULL, ticket );
}

extern "C" int
fd_ed25519_amd_submit_txns_keep( fd_ed25519_amd_t * e, ulong txn_cnt, uchar const * payload, uint const * txn_off,
                                 uint const * txn_sz, ulong payload_sz, schar * txn_err, uint * sig_base, schar * sig_err,
                                 ulong * txn_tag, ulong * sig_tag, ulong * desc_off, uchar * desc, ulong desc_cap,
                                 uint * keep, ulong * keep_cnt, ulong * ticket ) {
  return fd_ed25519_amd_submit_txns_budget( e, txn_cnt, payload, txn_off, txn_sz, payload_sz, txn_err, sig_base, sig_err, txn_tag,
                                            sig_tag, desc_off, desc, desc_cap, keep, keep_cnt, NULL, 0UL, NULL, NULL, NULL, ticket );
}

extern "C" int
fd_ed25519_amd_submit_txns_emit( fd_ed25519_amd_t * e, ulong txn_cnt, uchar const * payload, uint const * txn_off,
                                 uint const * txn_sz, ulong payload_sz, schar * txn_err, uint * sig_base, schar * sig_err,
                                 ulong * txn_tag, ulong * sig_tag, ulong * desc_off, uchar * desc, ulong desc_cap,
                                 uint * keep, ulong * keep_cnt, void * out, ulong out_cap, ulong * emit_off, uint * emit_sz,
                                 ulong * ticket ) {
  return fd_ed25519_amd_submit_txns_budget( e, txn_cnt, payload, txn_off, txn_sz, payload_sz, txn_err, sig_base, sig_err, txn_tag,
                                            sig_tag, desc_off, desc, desc_cap, keep, keep_cnt, out, out_cap, emit_off, emit_sz,
                                            NULL, ticket );
}

extern "C" int
fd_ed25519_amd_submit_txns_budget( fd_ed25519_amd_t * e, ulong txn_cnt, uchar const * payload, uint const * txn_off,
                                   uint const * txn_sz, ulong payload_sz, schar * txn_err, uint * sig_base, schar * sig_err,
                                   ulong * txn_tag, ulong * sig_tag, ulong * desc_off, uchar * desc, ulong desc_cap,
                                   uint * keep, ulong * keep_cnt, void * out, ulong out_cap, ulong * emit_off, uint * emit_sz,
                                   fd_txn_amd_budget_t * budget, ulong * ticket ) {
  if( !e || !ticket || !txn_cnt || KEEP_ARGS_BAD( keep, keep_cnt ) ) return FD_ED25519_AMD_ERR_INVAL;
  emit_args_t em;
  if( emit_args_check( &em, out, out_cap, emit_off, emit_sz, keep ) ) return FD_ED25519_AMD_ERR_INVAL;
  int rc = fd_amd_txn_args_check( e, txn_cnt, payload, txn_off, txn_sz, payload_sz, txn_err, sig_base, sig_err, sig_tag,
                                  desc_off, desc, desc_cap );
  if( rc ) return rc;
  if( !emit_cap_ok( em, txn_cnt, txn_sz, true ) ) return FD_ED25519_AMD_ERR_INVAL;
  slot_t * s = submit_slot( e, &rc );
  if( !s ) return rc;
  ulong bsz = 0, ns = 0;
  if( txns_chunk( e, txn_cnt, payload, txn_off, txn_sz, &bsz, &ns, []( ulong, uchar const *, ulong, ulong, ulong ){} ) != txn_cnt )
    return FD_ED25519_AMD_ERR_INVAL;   /* one chunk */
  s->a_dbase = 0UL;
  txn_outs_t o = { txn_err, sig_err, txn_tag, sig_tag, desc_off, desc, desc_cap, &s->a_dbase, budget };
  rc = submit_run( e, s, keep, keep_cnt, em, ticket, [&]() -> long { return stage_txns( e, s, txn_cnt, payload, txn_off, txn_sz, o, &ns ); } );
  /* pure host numbering: the one output a submit call writes */
  if( !rc && sig_base ) fd_ed25519_amd_txn_slots( txn_cnt, payload, txn_off, txn_sz, sig_base );
  return rc;
}

extern "C" int
fd_ed25519_amd_submit_txns_registered( fd_ed25519_amd_t * e, ulong txn_cnt, void const * const * txn, ulong const * txn_sz,
                                       schar * txn_err, uint * sig_base, schar * sig_err, ulong * txn_tag, ulong * sig_tag,
                                       ulong * desc_off, uchar * desc, ulong desc_cap, ulong * ticket ) {
  return fd_ed25519_amd_submit_txns_registered_keep( e, txn_cnt, txn, txn_sz, txn_err, sig_base, sig_err, txn_tag, sig_tag,
                                                     desc_off, desc, desc_cap, NULL, NULL, ticket );
}

extern "C" int
fd_ed25519_amd_submit_txns_registered_keep( fd_ed25519_amd_t * e, ulong txn_cnt, void const * const * txn,
                                            ulong const * txn_sz, schar * txn_err, uint * sig_base, schar * sig_err,
                                            ulong * txn_tag, ulong * sig_tag, ulong * desc_off, uchar * desc, ulong desc_cap,
                                            uint * keep, ulong * keep_cnt, ulong * ticket ) {
  return fd_ed25519_amd_submit_txns_registered_budget( e, txn_cnt, txn, txn_sz, txn_err, sig_base, sig_err, txn_tag, sig_tag,
                                                       desc_off, desc, desc_cap, keep, keep_cnt, NULL, 0UL, NULL, NULL, NULL,
                                                       ticket );
}

extern "C" int
fd_ed25519_amd_submit_txns_registered_emit( fd_ed25519_amd_t * e, ulong txn_cnt, void const * const * txn,
                                            ulong const * txn_sz, schar * txn_err, uint * sig_base, schar * sig_err,
                                            ulong * txn_tag, ulong * sig_tag, ulong * desc_off, uchar * desc, ulong desc_cap,
                                            uint * keep, ulong * keep_cnt, void * out, ulong out_cap, ulong * emit_off,
                                            uint * emit_sz, ulong * ticket ) {
  return fd_ed25519_amd_submit_txns_registered_budget( e, txn_cnt, txn, txn_sz, txn_err, sig_base, sig_err, txn_tag, sig_tag,
                                                       desc_off, desc, desc_cap, keep, keep_cnt, out, out_cap, emit_off, emit_sz,
                                                       NULL, ticket );
}

extern "C" int
fd_ed25519_amd_submit_txns_registered_budget( fd_ed25519_amd_t * e, ulong txn_cnt, void const * const * txn,
                                              ulong const * txn_sz, schar * txn_err, uint * sig_base, schar * sig_err,
                                              ulong * txn_tag, ulong * sig_tag, ulong * desc_off, uchar * desc, ulong desc_cap,
                                              uint * keep, ulong * keep_cnt, void * out, ulong out_cap, ulong * emit_off,
                                              uint * emit_sz, fd_txn_amd_budget_t * budget, ulong * ticket ) {
  if( !e || !ticket || !txn_cnt || txn_cnt > 0xFFFFFFFFUL || KEEP_ARGS_BAD( keep, keep_cnt ) ) return FD_ED25519_AMD_ERR_INVAL;
  if( txn_cnt > e->cap ) return FD_ED25519_AMD_ERR_INVAL;   /* one chunk (and it bounds the check's scratch) */
  emit_args_t em;
  if( emit_args_check( &em, out, out_cap, emit_off, emit_sz, keep ) ) return FD_ED25519_AMD_ERR_INVAL;
  reg_view_t view;
  std::vector<uint> slots( txn_cnt );
  int rc = txns_registered_check( e, view, txn_cnt, txn, txn_sz, txn_err, sig_base, sig_err, sig_tag, desc_off, desc,
                                  desc_cap, slots.data() );
  if( rc ) return rc;
  if( !emit_cap_ok( em, txn_cnt, txn_sz, true ) ) return FD_ED25519_AMD_ERR_INVAL;
  slot_t * s = submit_slot( e, &rc );
  if( !s ) return rc;
  /* one chunk: the layout over the whole submission, into the free slot's scratch */
  ulong ns = 0;
  if( fd_ed25519_amd_txn_gather_layout( txn_cnt, txn_sz, slots.data(), e->cap, e->blob_cap, slot_gather_dst( e, s ), &ns ) != txn_cnt )
    return FD_ED25519_AMD_ERR_INVAL;
  s->a_dbase = 0UL;
  txn_outs_t o = { txn_err, sig_err, txn_tag, sig_tag, desc_off, desc, desc_cap, &s->a_dbase, budget };
  rc = submit_run( e, s, keep, keep_cnt, em, ticket, [&]() -> long {
    return stage_txns_registered( e, s, view, txn_cnt, txn, txn_sz, slots.data(), o, &ns );
  } );
  /* pure host numbering: the one output a submit call writes */
  if( !rc && sig_base ) txns_sig_base( txn_cnt, slots.data(), sig_base );
  return rc;
}

/* Deliver the oldest submission, if it has finished (block: wait for it). */
static int
async_deliver( fd_ed25519_amd_t * e, ulong * ticket, bool block ) {
  if( !e || !ticket ) return FD_ED25519_AMD_ERR_INVAL;
  if( !e->a_cnt ) return FD_ED25519_AMD_ASYNC_NONE;
  slot_t * s = &e->slot[e->a_head];
  ulong const t = s->ticket;
  int rc = FD_ED25519_AMD_OK;
  if( !block ) {
    if( !e->poll_event ) {
      /* not finished yet: one load, no runtime call */
      if( __atomic_load_n( s->h_tick, __ATOMIC_ACQUIRE ) != t ) return FD_ED25519_AMD_ASYNC_NONE;
    } else {
      hipError_t q = hipEventQuery( s->done );
      if( q == hipErrorNotReady ) return FD_ED25519_AMD_ASYNC_NONE;
      if( q != hipSuccess ) rc = FD_ED25519_AMD_ERR_DEVICE;
    }
  }
  /* slot_drain waits for the slot's event whatever the word said: that wait
     is the barrier the outputs' visibility rests on, cheap once the chunk has
     finished.  It leaves the slot busy only when the runtime failed. */
  if( !rc ) rc = slot_drain( s );
  *ticket = t;
  if( rc && s->busy ) return engine_quiesce( e, rc );
  /* delivered, or the step guard tripped in this submission alone */
  e->a_head = (e->a_head + 1) % e->nslot; e->a_cnt--;
  return rc;
}

extern "C" int
fd_ed25519_amd_async_poll( fd_ed25519_amd_t * e, ulong * ticket ) { return async_deliver( e, ticket, false ); }

extern "C" int
fd_ed25519_amd_async_wait( fd_ed25519_amd_t * e, ulong * ticket ) { return async_deliver( e, ticket, true ); }

/* The engine's mode: every later call of this engine launches with it.  With
   nothing in flight: the synchronous calls drain their chunks, and while
   submissions are in flight the mode stays. */
extern "C" int
fd_ed25519_amd_set_mode( fd_ed25519_amd_t * e, int mode ) {
  if( !e || !fd_amd_mode_ok( mode ) || SYNC_REFUSED( e ) ) return FD_ED25519_AMD_ERR_INVAL;
  e->mode = mode;
  for( int k=0; k<FD_AMD_SLOT_MAX; k++ ) e->slot[k].strict = mode == FD_ED25519_AMD_MODE_STRICT;
  return FD_ED25519_AMD_OK;
}

extern "C" int
fd_ed25519_amd_mode( fd_ed25519_amd_t const * e ) {
  return e ? e->mode : FD_ED25519_AMD_ERR_INVAL;
}

/* The engine borrows w (NULL: gives its window back).  With nothing in
   flight every event recorded on the old window's behalf has fired, so it
   leaves with nothing queued. */
extern "C" int
fd_ed25519_amd_set_window( fd_ed25519_amd_t * e, fd_ed25519_amd_window_t * w ) {
  if( !e || e->a_cnt ) return FD_ED25519_AMD_ERR_INVAL;
  if( w && ( w->device != e->device || w->depth < e->cap || ( w->owner && w->owner != e ) ) ) return FD_ED25519_AMD_ERR_INVAL;
  if( e->win == w ) return FD_ED25519_AMD_OK;
  if( e->win ) { e->win->pend = NULL; e->win->owner = NULL; }
  e->win = w;
  if( w ) w->owner = e;
  return FD_ED25519_AMD_OK;
}

extern "C" fd_ed25519_amd_window_t *
fd_ed25519_amd_window( fd_ed25519_amd_t const * e ) { return e ? e->win : NULL; }

extern "C" int
fd_ed25519_amd_work_stats_dev( ulong n, void const * d_ws, uint * d_stats, void * stream ) {
  if( !n ) return FD_ED25519_AMD_OK;
  ws_layout_t L = fd_amd_ws_layout( n );
  uint8_t const * st = (uint8_t const *)d_ws + L.st;
  for( int k=0; k<3; k++ )
    HIPCHK( hipMemcpyAsync( d_stats + (ulong)k*n, st + 4UL*(ulong)k*L.N, 4UL*n, hipMemcpyDeviceToDevice, (hipStream_t)stream ) );
  return FD_ED25519_AMD_OK;
}

extern "C" int
fd_ed25519_amd_tags_dev( ulong n, void const * d_ws, ulong * d_tag, void * stream ) {
  if( n > 0xFFFFFFFFUL ) return FD_ED25519_AMD_ERR_INVAL;
  if( !n ) return FD_ED25519_AMD_OK;
  if( !d_ws || !d_tag || ((uintptr_t)d_tag & 7UL) ) return FD_ED25519_AMD_ERR_INVAL;
  if( fd_amd_launch_tag_out( d_tag, d_ws, n, (hipStream_t)stream ) ) return FD_ED25519_AMD_ERR_DEVICE;
  return FD_ED25519_AMD_OK;
}

extern "C" int
fd_ed25519_amd_txn_tags_dev( ulong txn_cnt, uint const * d_tbase, void const * d_ws, ulong * d_txn_tag, void * stream ) {
  if( txn_cnt > 0xFFFFFFFFUL ) return FD_ED25519_AMD_ERR_INVAL;
  if( !txn_cnt ) return FD_ED25519_AMD_OK;
  if( !d_tbase || !d_ws || !d_txn_tag || ((uintptr_t)d_txn_tag & 7UL) ) return FD_ED25519_AMD_ERR_INVAL;
  if( fd_amd_launch_tag_gather( d_txn_tag, d_ws, (uint32_t)txn_cnt, d_tbase, (hipStream_t)stream ) ) return FD_ED25519_AMD_ERR_DEVICE;
  return FD_ED25519_AMD_OK;
}

extern "C" ulong
fd_ed25519_amd_keep_scratch_footprint( ulong n ) {
  return n > (ulong)FD_AMD_KEEP_MAX ? 0UL : (ulong)fd_amd_keep_layout( n ).total;
}

extern "C" int
fd_ed25519_amd_keep_dev( ulong n, schar const * d_err, ulong const * d_tag, uint * d_keep, ulong * d_keep_cnt,
                         void * d_scratch, ulong salt, void * stream ) {
  if( n > (ulong)FD_AMD_KEEP_MAX || !d_keep_cnt || ((uintptr_t)d_keep_cnt & 7UL) ) return FD_ED25519_AMD_ERR_INVAL;
  if( n && ( !d_err || !d_tag || !d_keep || !d_scratch || ((uintptr_t)d_tag & 7UL) || ((uintptr_t)d_keep & 3UL) ||
             ((uintptr_t)d_scratch & 255UL) ) )
    return FD_ED25519_AMD_ERR_INVAL;
  if( fd_amd_launch_keep( (uint32_t)n, (int8_t const *)d_err, (uint64_t const *)d_tag, NULL, NULL, (uint32_t *)d_keep,
                          (uint64_t *)d_keep_cnt, d_scratch, salt, (hipStream_t)stream ) )
    return FD_ED25519_AMD_ERR_DEVICE;
  return FD_ED25519_AMD_OK;
}

extern "C" ulong
fd_ed25519_amd_emit_scratch_footprint( ulong n ) {
  return n > (ulong)FD_AMD_KEEP_MAX ? 0UL : (ulong)fd_amd_emit_layout( n ).total;
}

/* The argument check both device-resident emit forms share. */
static bool
emit_dev_args_ok( ulong n, void const * d_keep, void const * d_keep_cnt, void const * d_out, ulong out_cap,
                  void const * d_emit_off, void const * d_emit_sz, void const * d_scratch ) {
  if( n > (ulong)FD_AMD_KEEP_MAX || !d_keep_cnt || ((uintptr_t)d_keep_cnt & 7UL) || !d_emit_off || ((uintptr_t)d_emit_off & 7UL) ||
      !d_scratch || ((uintptr_t)d_scratch & 255UL) || ( out_cap && !d_out ) || ((uintptr_t)d_out & 63UL) )
    return false;
  return !n || ( d_keep && !((uintptr_t)d_keep & 3UL) && d_emit_sz && !((uintptr_t)d_emit_sz & 3UL) );
}

extern "C" int
fd_ed25519_amd_emit_dev( ulong n, uchar const * d_pub, uchar const * d_sig, uint const * d_msg_off, uint const * d_msg_sz,
                         uchar const * d_blob, uint const * d_keep, ulong const * d_keep_cnt, void * d_out, ulong out_cap,
                         ulong * d_emit_off, uint * d_emit_sz, void * d_scratch, void * stream ) {
  if( !emit_dev_args_ok( n, d_keep, d_keep_cnt, d_out, out_cap, d_emit_off, d_emit_sz, d_scratch ) ||
      ( n && ( !d_pub || !d_sig || !d_msg_off || !d_msg_sz || !d_blob ) ) )
    return FD_ED25519_AMD_ERR_INVAL;
  if( fd_amd_launch_emit_sig( (uint32_t)n, d_pub, d_sig, d_msg_off, d_msg_sz, d_blob, d_keep, (uint64_t const *)d_keep_cnt, d_out,
                              out_cap, (uint64_t *)d_emit_off, d_emit_sz, d_scratch, 0u, (hipStream_t)stream ) )
    return FD_ED25519_AMD_ERR_DEVICE;
  return FD_ED25519_AMD_OK;
}

extern "C" int
fd_txn_amd_emit_dev( ulong txn_cnt, uchar const * d_payload, uint const * d_txn_off, uint const * d_txn_sz,
                     ulong const * d_desc_off, uchar const * d_desc, uint const * d_keep, ulong const * d_keep_cnt, void * d_out,
                     ulong out_cap, ulong * d_emit_off, uint * d_emit_sz, void * d_scratch, void * stream ) {
  if( !emit_dev_args_ok( txn_cnt, d_keep, d_keep_cnt, d_out, out_cap, d_emit_off, d_emit_sz, d_scratch ) ||
      ( txn_cnt && ( !d_payload || !d_txn_off || !d_txn_sz || !d_desc_off || ((uintptr_t)d_desc_off & 7UL) || !d_desc ) ) )
    return FD_ED25519_AMD_ERR_INVAL;
  if( fd_amd_launch_emit_txn( (uint32_t)txn_cnt, d_payload, d_txn_off, d_txn_sz, (uint64_t const *)d_desc_off, d_desc, d_keep,
                              (uint64_t const *)d_keep_cnt, d_out, out_cap, (uint64_t *)d_emit_off, d_emit_sz, d_scratch, 0u,
                              (hipStream_t)stream ) )
    return FD_ED25519_AMD_ERR_DEVICE;
  return FD_ED25519_AMD_OK;
}

extern "C" int
fd_ed25519_amd_debug_digits_dev( ulong n, void const * d_ws, ushort * d_dig, int * d_top, void * stream ) {
  if( !n ) return FD_ED25519_AMD_OK;
  ws_layout_t L = fd_amd_ws_layout( n );
  uint8_t const * ws = (uint8_t const *)d_ws;
  if( fd_amd_launch_digits_dense( (uint32_t)n, d_ws, d_dig, (hipStream_t)stream ) ) return FD_ED25519_AMD_ERR_DEVICE;
  HIPCHK( hipMemcpyAsync( d_top, ws + L.top, 4UL*n,   hipMemcpyDeviceToDevice, (hipStream_t)stream ) );
  return FD_ED25519_AMD_OK;
}

extern "C" int
fd_ed25519_amd_debug_points_dev( ulong n, void const * d_ws, int * d_A, int * d_R, uchar * d_ds, void * stream ) {
  if( !n ) return FD_ED25519_AMD_OK;
  if( !d_ws || !d_A || !d_R || !d_ds ) return FD_ED25519_AMD_ERR_INVAL;
  ws_layout_t L = fd_amd_ws_layout( n );
  uint8_t const * ws = (uint8_t const *)d_ws;
  /* the planes are [limb][L.N]: one copy per limb packs them to [limb][n] (a debug path) */
  for( ulong k=0; k<30UL; k++ )
    HIPCHK( hipMemcpyAsync( d_A + k*n, ws + L.A + 4UL*k*L.N, 4UL*n, hipMemcpyDeviceToDevice, (hipStream_t)stream ) );
  for( ulong k=0; k<20UL; k++ )
    HIPCHK( hipMemcpyAsync( d_R + k*n, ws + L.R + 4UL*k*L.N, 4UL*n, hipMemcpyDeviceToDevice, (hipStream_t)stream ) );
  HIPCHK( hipMemcpyAsync( d_ds, ws + L.ds, 2UL*n, hipMemcpyDeviceToDevice, (hipStream_t)stream ) );
  return FD_ED25519_AMD_OK;
}

extern "C" int
fd_ed25519_amd_debug_rprime_dev( ulong n, void const * d_ws, int kind, int * d_xyz, void * stream ) {
  if( n > 0xFFFFFFFFUL || kind < FD_ED25519_AMD_DSM_DEFAULT || kind > FD_ED25519_AMD_DSM_K_DSMP ) return FD_ED25519_AMD_ERR_INVAL;
  if( !n ) return FD_ED25519_AMD_OK;
  if( !d_ws || !d_xyz ) return FD_ED25519_AMD_ERR_INVAL;
  if( fd_amd_launch_rprime( (uint32_t)n, d_ws, kind, d_xyz, (hipStream_t)stream ) ) return FD_ED25519_AMD_ERR_DEVICE;
  return FD_ED25519_AMD_OK;
}

/* ------------------------------------------------------------------ */
/* drop-in reference API                                                */

/* One engine per calling thread (the reference is reentrant with one
   fd_sha512_t per thread, fd_frank_verify.c:121-123), freed by a
   pthread-key destructor when the thread exits.  The reference boots N
   verify tiles as threads of one process (fd_frank_main.c:118-143), so the
   engine's device is a per-thread choice: the thread's own
   (fd_ed25519_amd_dropin_set_device), else FD_ED25519_AMD_DEVICE, else
   round robin over the GPUs local to the NUMA node of the CPU the thread
   first verifies on (fd_ed25519_amd_dropin_pick). */
namespace {
struct dropin_t { fd_ed25519_amd_t * eng; ulong blob; int want; int dev; };
pthread_key_t  dropin_key;
pthread_once_t dropin_once = PTHREAD_ONCE_INIT;
void dropin_free( void * p ) {
  dropin_t * d = (dropin_t *)p;
  if( d->eng ) fd_ed25519_amd_delete( d->eng );
  free( d );
}
void dropin_key_init( void ) { (void)pthread_key_create( &dropin_key, dropin_free ); }
dropin_t * dropin_self( void ) {
  (void)pthread_once( &dropin_once, dropin_key_init );
  dropin_t * d = (dropin_t *)pthread_getspecific( dropin_key );
  if( !d ) {
    d = (dropin_t *)calloc( 1, sizeof(dropin_t) );
    if( !d || pthread_setspecific( dropin_key, d ) ) { free( d ); return NULL; }
    d->want = FD_ED25519_AMD_DROPIN_AUTO; d->dev = -1;
  }
  return d;
}
/* threads given a default device so far, per NUMA node of their CPU (the
   last counter takes unknown and out-of-range nodes) */
std::atomic<ulong> dropin_ordinal[65];

/* The default device of a thread that set none. */
int dropin_default_device( void ) {
  char const * dv = getenv( "FD_ED25519_AMD_DEVICE" );
  if( dv && *dv ) return atoi( dv );
  int cnt = 0;
  if( hipGetDeviceCount( &cnt ) != hipSuccess || cnt <= 0 ) { (void)hipGetLastError(); return 0; }
  int node_of[FD_ED25519_AMD_DROPIN_DEV_MAX];
  cnt = std::min( cnt, (int)FD_ED25519_AMD_DROPIN_DEV_MAX );
  for( int k=0; k<cnt; k++ ) node_of[k] = fd_ed25519_amd_device_numa_node( k );
  unsigned cpu = 0, node = 0;
  int const cpu_node = syscall( SYS_getcpu, &cpu, &node, NULL ) ? -1 : (int)node;
  ulong const o = dropin_ordinal[ cpu_node >= 0 && cpu_node < 64 ? cpu_node : 64 ].fetch_add( 1UL );
  return fd_ed25519_amd_dropin_pick( node_of, cnt, cpu_node, o );
}
}

extern "C" int
fd_ed25519_amd_dropin_pick( int const * dev_node, int dev_cnt, int cpu_node, ulong ordinal ) {
  if( dev_cnt <= 0 || !dev_node ) return 0;
  int local = 0;
  if( cpu_node >= 0 ) for( int k=0; k<dev_cnt; k++ ) local += dev_node[k] == cpu_node;
  if( !local ) return (int)(ordinal % (ulong)dev_cnt);
  ulong j = ordinal % (ulong)local;
  for( int k=0; k<dev_cnt; k++ ) if( dev_node[k] == cpu_node && !j-- ) return k;
  return 0;   /* not reached */
}

extern "C" int
fd_ed25519_amd_dropin_set_device( int device ) {
  if( device < FD_ED25519_AMD_DROPIN_AUTO ) return FD_ED25519_AMD_ERR_INVAL;
  if( device >= 0 ) {
    int cnt = 0;
    if( hipGetDeviceCount( &cnt ) != hipSuccess ) { (void)hipGetLastError(); return FD_ED25519_AMD_ERR_DEVICE; }
    if( device >= cnt ) return FD_ED25519_AMD_ERR_INVAL;
  }
  dropin_t * d = dropin_self();
  if( !d ) return FD_ED25519_AMD_ERR_INVAL;
  d->want = device;
  return FD_ED25519_AMD_OK;
}

extern "C" int
fd_ed25519_amd_dropin_device( void ) {
  dropin_t * d = dropin_self();
  return d && d->eng ? d->dev : -1;
}

extern "C" int
fd_ed25519_verify( void const * msg, ulong sz, void const * sig, void const * public_key, fd_sha512_t * sha ) {
  (void)sha;   /* scratch of the reference; hashing happens on the GPU */
  dropin_t * d = dropin_self();
  if( !d ) {
    fprintf( stderr, "fd_ed25519_verify: out of memory\n" );
    abort();
  }
  if( sz > 0xFFFFFFFFUL - 4096UL ) {
    fprintf( stderr, "fd_ed25519_verify: message of %lu bytes exceeds the engine's 32-bit offsets\n", sz );
    abort();
  }
  /* the thread's device: its own choice, else the default picked once */
  int const dev = d->want >= 0 ? d->want : d->dev >= 0 ? d->dev : dropin_default_device();
  /* the engine grows when a message exceeds its staging (the reference
     accepts any size) and moves when the thread's device changed */
  if( !d->eng || sz > d->blob || dev != d->dev ) {
    ulong want = std::max( d->eng ? d->blob : 0UL, 64UL*FD_ED25519_AMD_MSG_MAX );
    while( want < sz ) want <<= 1;
    if( d->eng ) { fd_ed25519_amd_delete( d->eng ); d->eng = NULL; }
    d->eng = fd_ed25519_amd_new( dev, 64UL, want );
    if( !d->eng ) {
      fprintf( stderr, "fd_ed25519_verify: no usable MI355X/HIP device %d; this library has no CPU path\n", dev );
      abort();
    }
    d->blob = want; d->dev = dev;
  }
  static uint8_t const zero = 0;
  uint32_t off = 0, s32 = (uint32_t)sz;
  schar err = 0;
  int rc = fd_ed25519_amd_verify_soa( d->eng, 1UL, (uchar const *)public_key, (uchar const *)sig, &off, &s32,
                                      sz ? (uchar const *)msg : &zero, sz, &err );
  if( rc ) { fprintf( stderr, "fd_ed25519_verify: device error %d\n", rc ); abort(); }
  return (int)err;
}

extern "C" char const *
fd_ed25519_strerror( int err ) {
  switch( err ) {
  case FD_ED25519_SUCCESS:    return "success";
  case FD_ED25519_ERR_SIG:    return "bad signature";
  case FD_ED25519_ERR_PUBKEY: return "bad public key";
  case FD_ED25519_ERR_MSG:    return "bad message";
  default: break;
  }
  return "unknown";
}

extern "C" char const *
fd_ed25519_amd_version( void ) {
  return "fd_ed25519_amd 0.3 (gfx950; k_prep/k_decomp/k_dsm + k_front/k_dsm8/k_dsm4, txn front end, verify tile, multi-device, GPU signer)";
}

#ifdef FD_AMD_DIAG
#include <time.h>
#include <x86intrin.h>
#include <algorithm>
/* Diagnostics build only.  Latency-path A/B (profiles/r04_latency_ab.txt):
   one n-signature batch resident in HBM, verified `iters` times per way of
   launching and waiting, each call timed on the host clock:
     mode 0  k_front + k_dsm8 launched on a stream, hipEventSynchronize
     mode 1  the same launches, host spins on the verdicts k_dsm8 writes
             into mapped memory
     mode 2  the two launches captured once into a hipGraph, hipGraphLaunch
             + hipEventSynchronize
     mode 3  hipGraphLaunch + spin on the mapped verdicts
   out[4*m + 0..3] = p50 / p99 / min us of mode m and its GPU time (events
   around the launches, p50).  Every call's verdicts must equal the first
   call's (checked; ERR_DEVICE otherwise). */
extern "C" int
fd_amd_latency_ab( int device, uint32_t n, uint8_t const * pub, uint8_t const * sig, uint32_t const * off,
                   uint32_t const * sz, uint8_t const * blob, uint64_t blob_sz, uint32_t iters, double * out ) {
  if( !n || !iters || !out || !fd_amd_uses_latency_path( n, 0 ) ) return FD_ED25519_AMD_ERR_INVAL;
  if( hipSetDevice( device ) != hipSuccess ) return FD_ED25519_AMD_ERR_DEVICE;
  int rc = FD_ED25519_AMD_ERR_DEVICE;
  uint8_t * d_in = NULL, * d_ws = NULL; int8_t * d_err = NULL, * h_out = NULL, * d_out = NULL;
  hipStream_t st = NULL; hipEvent_t e0 = NULL, e1 = NULL, ed = NULL;
  hipGraph_t g = NULL; hipGraphExec_t ge = NULL;
  ulong const in_sz = 104UL*n + blob_sz;
  std::vector<int8_t> first( n );
  std::vector<double> t( iters ), gt( iters );
  ws_layout_t const L = fd_amd_ws_layout( n );
  uint8_t * p_pub, * p_sig, * p_blob; uint32_t * p_off, * p_sz;
  auto now = []() { struct timespec ts; clock_gettime( CLOCK_MONOTONIC, &ts ); return (double)ts.tv_sec * 1e6 + (double)ts.tv_nsec * 1e-3; };
  if( hipMalloc( (void **)&d_in, in_sz ) != hipSuccess || hipMalloc( (void **)&d_ws, L.total ) != hipSuccess ||
      hipMalloc( (void **)&d_err, n ) != hipSuccess ||
      hipHostMalloc( (void **)&h_out, n, hipHostMallocMapped | hipHostMallocCoherent ) != hipSuccess ||
      hipHostGetDevicePointer( (void **)&d_out, h_out, 0 ) != hipSuccess ||
      hipStreamCreateWithFlags( &st, hipStreamNonBlocking ) != hipSuccess ||
      hipEventCreate( &e0 ) != hipSuccess || hipEventCreate( &e1 ) != hipSuccess || hipEventCreate( &ed ) != hipSuccess )
    goto done;
  p_pub = d_in; p_sig = d_in + 32UL*n; p_off = (uint32_t *)(d_in + 96UL*n); p_sz = (uint32_t *)(d_in + 100UL*n); p_blob = d_in + 104UL*n;
  if( hipMemcpy( p_pub, pub, 32UL*n, hipMemcpyHostToDevice ) != hipSuccess ||
      hipMemcpy( p_sig, sig, 64UL*n, hipMemcpyHostToDevice ) != hipSuccess ||
      hipMemcpy( p_off, off, 4UL*n, hipMemcpyHostToDevice ) != hipSuccess ||
      hipMemcpy( p_sz, sz, 4UL*n, hipMemcpyHostToDevice ) != hipSuccess ||
      ( blob_sz && hipMemcpy( p_blob, blob, blob_sz, hipMemcpyHostToDevice ) != hipSuccess ) ) goto done;
  /* the graph: the same two launches, captured */
  if( hipStreamBeginCapture( st, hipStreamCaptureModeThreadLocal ) != hipSuccess ) goto done;
  if( fd_amd_launch_verify( n, p_pub, p_sig, p_off, p_sz, p_blob, d_err, d_ws, st, 0, NULL, NULL, 0, d_out ) ) {
    (void)hipStreamEndCapture( st, &g ); goto done;
  }
  if( hipStreamEndCapture( st, &g ) != hipSuccess || hipGraphInstantiate( &ge, g, NULL, NULL, 0 ) != hipSuccess ) goto done;
  for( int m=0; m<4; m++ ) {
    bool const graph = m >= 2, spin = m & 1;
    for( uint32_t it=0; it<iters + 8u; it++ ) {   /* 8 untimed warm-up calls */
      memset( h_out, 0x7f, n );
      double const a = now();
      if( hipEventRecord( e0, st ) != hipSuccess ) goto done;
      if( graph ) { if( hipGraphLaunch( ge, st ) != hipSuccess ) goto done; }
      else if( fd_amd_launch_verify( n, p_pub, p_sig, p_off, p_sz, p_blob, d_err, d_ws, st, 0, NULL, NULL, 0, d_out ) ) goto done;
      if( hipEventRecord( e1, st ) != hipSuccess ) goto done;
      if( spin ) {
        /* every verdict lands in mapped memory; wait for the last unwritten one */
        for( uint32_t j=0; j<n; ) { if( ((int8_t volatile *)h_out)[j] != (int8_t)0x7f ) j++; else _mm_pause(); }
      } else if( hipEventSynchronize( e1 ) != hipSuccess ) goto done;
      double const b = now();
      if( hipEventSynchronize( e1 ) != hipSuccess ) goto done;
      float ms = 0.f;
      if( hipEventElapsedTime( &ms, e0, e1 ) != hipSuccess ) goto done;
      if( m == 0 && it == 0 ) memcpy( first.data(), h_out, n );
      else if( memcmp( first.data(), h_out, n ) ) { fprintf( stderr, "fd_amd_latency_ab: verdicts differ (mode %d call %u)\n", m, it ); goto done; }
      if( it >= 8u ) { t[it - 8u] = b - a; gt[it - 8u] = 1e3 * (double)ms; }
    }
    std::sort( t.begin(), t.end() ); std::sort( gt.begin(), gt.end() );
    out[4*m + 0] = t[iters / 2]; out[4*m + 1] = t[std::min( (ulong)iters - 1UL, (ulong)(0.99 * iters) )];
    out[4*m + 2] = t[0]; out[4*m + 3] = gt[iters / 2];
  }
  rc = FD_ED25519_AMD_OK;
done:
  if( st ) (void)hipStreamSynchronize( st );
  if( ge ) (void)hipGraphExecDestroy( ge );
  if( g ) (void)hipGraphDestroy( g );
  if( e0 ) (void)hipEventDestroy( e0 );
  if( e1 ) (void)hipEventDestroy( e1 );
  if( ed ) (void)hipEventDestroy( ed );
  if( st ) (void)hipStreamDestroy( st );
  if( h_out ) (void)hipHostFree( h_out );
  if( d_in ) (void)hipFree( d_in );
  if( d_ws ) (void)hipFree( d_ws );
  if( d_err ) (void)hipFree( d_err );
  return rc;
}
#endif /* FD_AMD_DIAG */
