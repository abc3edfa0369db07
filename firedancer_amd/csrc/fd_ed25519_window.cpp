/* firedancer_amd/csrc/fd_ed25519_window.cpp
 *
 * The dedup window object (include/fd_ed25519_amd.h, "The dedup window"):
 * creation, the rule as pure host code on a host-only window, the
 * device-resident filter call, export and import.  The kernels are in
 * fd_ed25519_window.h; an engine's use of an attached window is in
 * fd_ed25519_engine.cpp (slot_keep).
 *
 * The host-only window keeps the device window's data structure -- a ring,
 * a count, and a map of stamped keys that is never deleted from and is
 * rebuilt when the items offered since the last rebuild exceed depth -- so
 * that one description covers both; the reference's tile keeps a ring plus a
 * hash set for the same job (fd_tcache, src/tango/tcache/fd_tcache.h).
 */
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <sys/random.h>
#include <time.h>
#include <vector>

#include "../../include/fd_ed25519_amd.h"
#include "fd_ed25519_kernels.h"

#define HIPCHK( x ) do { hipError_t _e = (x); if( _e != hipSuccess ) {                          \
    fprintf( stderr, "fd_ed25519_amd: %s failed: %s (%s:%d)\n", #x, hipGetErrorString( _e ),     \
             __FILE__, __LINE__ );                                                              \
    return FD_ED25519_AMD_ERR_DEVICE; } } while(0)

#include "fd_ed25519_engine.h"

typedef fd_ed25519_amd_window_t win_t;

/* keep_home of fd_ed25519_keep.h on the host: the two windows need not share
   a slot function (no output depends on it), but one is enough */
static inline ulong
win_home( ulong tag, ulong salt, ulong mask ) {
  ulong x = tag ^ salt;
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9UL;
  x ^= x >> 27; x *= 0x94d049bb133111ebUL;
  x ^= x >> 31;
  return x & mask;
}

/* The slot of t in the host map: its own, or the empty one that ends its probe. */
static inline ulong
win_find( win_t const * w, ulong t ) {
  ulong const mask = w->cap - 1UL;
  ulong s = win_home( t, w->salt, mask );
  while( w->h_key[s] && w->h_key[s] != t ) s = (s + 1UL) & mask;
  return s;
}

static void
win_host_rebuild( win_t * w ) {
  memset( w->h_key,   0, 8UL*w->cap );
  memset( w->h_stamp, 0, 8UL*w->cap );
  for( ulong q = w->h_head > w->depth ? w->h_head - w->depth : 0UL; q < w->h_head; q++ ) {
    ulong const t = w->h_ring[q % w->depth], s = win_find( w, t );
    w->h_key[s] = t; w->h_stamp[s] = q + 1UL;
  }
}

/* Wait for whatever was last queued on the window. */
static int
win_wait( win_t * w ) {
  if( w->pend ) { HIPCHK( hipEventSynchronize( w->pend ) ); w->pend = NULL; }
  return FD_ED25519_AMD_OK;
}

extern "C" {

fd_ed25519_amd_window_t *
fd_ed25519_amd_window_new( int device, ulong depth, ulong salt ) {
  if( !depth || depth > FD_ED25519_AMD_WINDOW_DEPTH_MAX ) return NULL;   /* before anything touches a device */
  win_t * w = (win_t *)calloc( 1, sizeof(win_t) );
  if( !w ) return NULL;
  if( !salt && getrandom( &salt, sizeof(salt), 0 ) != (ssize_t)sizeof(salt) ) {
    struct timespec ts; (void)clock_gettime( CLOCK_MONOTONIC, &ts );
    salt = ( (ulong)ts.tv_sec * 1000000007UL ) ^ ( (ulong)ts.tv_nsec << 21 ) ^ (ulong)(uintptr_t)w;
  }
  fd_amd_win_layout_t L = fd_amd_win_layout( depth );
  w->device = device < 0 ? -1 : device; w->depth = depth; w->salt = salt; w->cap = L.cap;
  if( device < 0 ) {
    w->h_ring  = (ulong *)calloc( depth, 8UL );
    w->h_key   = (ulong *)calloc( L.cap, 8UL );
    w->h_stamp = (ulong *)calloc( L.cap, 8UL );
    if( !w->h_ring || !w->h_key || !w->h_stamp ) { fd_ed25519_amd_window_delete( w ); return NULL; }
    return w;
  }
  int cnt = 0;
  if( hipGetDeviceCount( &cnt ) != hipSuccess || device >= cnt || hipSetDevice( device ) != hipSuccess ||
      hipMalloc( (void **)&w->d_state, L.total ) != hipSuccess ) {
    w->d_state = NULL; fd_ed25519_amd_window_delete( w ); return NULL;
  }
  if( hipEventCreateWithFlags( &w->own_ev, hipEventDisableTiming ) != hipSuccess ) {
    w->own_ev = NULL; fd_ed25519_amd_window_delete( w ); return NULL;
  }
  if( fd_ed25519_amd_window_import( w, NULL, 0UL ) ) { fd_ed25519_amd_window_delete( w ); return NULL; }
  return w;
}

void
fd_ed25519_amd_window_delete( fd_ed25519_amd_window_t * w ) {
  if( !w ) return;
  if( w->owner ) { w->owner->win = NULL; w->owner = NULL; }
  if( w->device >= 0 ) {
    (void)hipSetDevice( w->device );
    (void)win_wait( w );
    if( w->own_ev  ) (void)hipEventDestroy( w->own_ev );
    if( w->d_state ) (void)hipFree( w->d_state );
  }
  free( w->h_ring ); free( w->h_key ); free( w->h_stamp );
  free( w );
}

ulong
fd_ed25519_amd_window_depth( fd_ed25519_amd_window_t const * w ) { return w ? w->depth : 0UL; }

/* The rule on a host-only window.  One pass: an item's tag is looked up in
   the map; a stamp within depth of the count the submission started with
   means live -- and a stamp beyond that count an insert of this very
   submission, today's in-batch duplicate -- and drops the item; otherwise the
   tag takes the next ring position and the stamp that goes with it. */
ulong
fd_ed25519_amd_window_keep( fd_ed25519_amd_window_t * w, ulong n, schar const * err, ulong const * tag, uint * keep ) {
  if( !w || w->device >= 0 || n > w->depth || ( n && ( !err || !tag ) ) ) return ~0UL;
  if( !n ) return 0UL;
  if( w->since + n > w->depth ) { win_host_rebuild( w ); w->since = n; }
  else w->since += n;
  ulong const H = w->h_head;
  ulong cnt = 0UL, r = 0UL;
  for( ulong i=0; i<n; i++ ) {
    if( err[i] ) continue;
    ulong const t = tag[i];
    if( t ) {
      ulong const s = win_find( w, t );
      if( w->h_key[s] && w->h_stamp[s] - 1UL + w->depth >= H ) continue;
      w->h_key[s] = t; w->h_stamp[s] = H + r + 1UL;
      w->h_ring[(H + r) % w->depth] = t;
      r++;
    }
    if( keep ) keep[cnt] = (uint)i;
    cnt++;
  }
  w->h_head = H + r;
  return cnt;
}

ulong
fd_ed25519_amd_window_keep_scratch_footprint( ulong n ) {
  return n > (ulong)FD_AMD_KEEP_MAX ? 0UL : (ulong)fd_amd_win_scratch( n ).total;
}

int
fd_ed25519_amd_window_keep_dev( fd_ed25519_amd_window_t * w, ulong n, schar const * d_err, ulong const * d_tag, uint * d_keep,
                                ulong * d_keep_cnt, void * d_scratch, void * stream ) {
  if( !w || w->device < 0 || w->owner || n > w->depth || !d_keep_cnt || ((uintptr_t)d_keep_cnt & 7UL) )
    return FD_ED25519_AMD_ERR_INVAL;
  if( n && ( !d_err || !d_tag || !d_keep || !d_scratch || ((uintptr_t)d_tag & 7UL) || ((uintptr_t)d_keep & 3UL) ||
             ((uintptr_t)d_scratch & 255UL) ) )
    return FD_ED25519_AMD_ERR_INVAL;
  fd_amd_win_dev_t d; fd_amd_win_dev_t const * dp = NULL;
  if( n ) { d = fd_amd_window_arm( w, n, w->own_ev ); dp = &d; }
  if( fd_amd_launch_keep_win( (uint32_t)n, (int8_t const *)d_err, (uint64_t const *)d_tag, NULL, NULL, (uint32_t *)d_keep,
                              (uint64_t *)d_keep_cnt, d_scratch, w->salt, dp, (hipStream_t)stream ) )
    return FD_ED25519_AMD_ERR_DEVICE;
  return FD_ED25519_AMD_OK;
}

ulong
fd_ed25519_amd_window_export( fd_ed25519_amd_window_t * w, ulong * tags ) {
  if( !w ) return ~0UL;
  ulong H = w->h_head;
  ulong const * ring = w->h_ring;
  std::vector<ulong> tmp;
  if( w->device >= 0 ) {
    fd_amd_win_layout_t L = fd_amd_win_layout( w->depth );
    tmp.resize( w->depth );
    if( hipSetDevice( w->device ) != hipSuccess || win_wait( w ) ||
        hipMemcpy( &H, w->d_state + L.head + 8UL*( w->seq & 1UL ), 8UL, hipMemcpyDeviceToHost ) != hipSuccess ||
        hipMemcpy( tmp.data(), w->d_state + L.ring, 8UL*w->depth, hipMemcpyDeviceToHost ) != hipSuccess )
      return ~0UL;
    ring = tmp.data();
  }
  ulong const lo = H > w->depth ? H - w->depth : 0UL;
  if( tags ) for( ulong q=lo; q<H; q++ ) tags[q - lo] = ring[q % w->depth];
  return H - lo;
}

int
fd_ed25519_amd_window_import( fd_ed25519_amd_window_t * w, ulong const * tags, ulong cnt ) {
  if( !w || cnt > w->depth || ( cnt && !tags ) ) return FD_ED25519_AMD_ERR_INVAL;
  for( ulong q=0; q<cnt; q++ ) if( !tags[q] ) return FD_ED25519_AMD_ERR_INVAL;
  if( w->owner && fd_ed25519_amd_async_in_flight( w->owner ) ) return FD_ED25519_AMD_ERR_INVAL;
  w->since = 0UL;
  if( w->device < 0 ) {
    if( cnt ) memcpy( w->h_ring, tags, 8UL*cnt );
    w->h_head = cnt;
    win_host_rebuild( w );
    return FD_ED25519_AMD_OK;
  }
  fd_amd_win_layout_t L = fd_amd_win_layout( w->depth );
  HIPCHK( hipSetDevice( w->device ) );
  if( win_wait( w ) ) return FD_ED25519_AMD_ERR_DEVICE;
  if( cnt ) HIPCHK( hipMemcpy( w->d_state + L.ring, tags, 8UL*cnt, hipMemcpyHostToDevice ) );
  HIPCHK( hipMemcpy( w->d_state + L.head + 8UL*( w->seq & 1UL ), &cnt, 8UL, hipMemcpyHostToDevice ) );
  w->since = w->depth + 1UL;   /* arm( 0 ) below: a rebuild, after which since is 0 */
  fd_amd_win_dev_t d = fd_amd_window_arm( w, 0UL, NULL );
  if( fd_amd_launch_win_rebuild( &d, NULL ) ) return FD_ED25519_AMD_ERR_DEVICE;
  HIPCHK( hipStreamSynchronize( NULL ) );
  return FD_ED25519_AMD_OK;
}

} /* extern "C" */
