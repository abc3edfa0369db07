/* tests/c/emit_host_check.c -- the host output-frame functions
   (fd_ed25519_amd_emit, fd_txn_amd_emit and the two bounds) run on a case
   file under the sanitizers.  tests/test_emit_cpu.py builds this file and
   fd_ed25519_host.cpp with -fsanitize=address,undefined and writes the cases
   (the inputs and the byte image the model expects).  Every input and output
   buffer is a heap block of exactly its size, so a read or a store one byte
   out of bounds stops the program.

   Case file, every integer a little-endian u64:
     "FDEMIT01", case count, then per case
       family (0 signatures, 1 transactions), item count, keep_cnt, keep[keep_cnt]
       per item: signatures    sz, pub[32], sig[64], msg[sz]
                 transactions  P, F, payload[P], desc[F]
       total, emit_off[keep_cnt + 1], emit_sz[keep_cnt], image[total]
   The image is the expected extent after a call on a buffer of 0xA5.

   usage: emit_host_check CASES */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fd_ed25519_amd.h"
#include "fd_txn_amd.h"

#define FILL (0xA5)

static FILE * f;

static ulong
rd( void ) {
  uchar b[8]; ulong v = 0UL;
  if( fread( b, 1, 8, f ) != 8 ) { fprintf( stderr, "short case file\n" ); exit( 2 ); }
  for( int k=7; k>=0; k-- ) v = ( v << 8 ) | b[k];
  return v;
}

/* a heap block of exactly sz bytes read from the file (sz == 0: NULL, which nobody may read) */
static uchar *
rd_bytes( ulong sz ) {
  if( !sz ) return NULL;
  uchar * p = malloc( sz );
  if( !p || fread( p, 1, sz, f ) != sz ) { fprintf( stderr, "short case file\n" ); exit( 2 ); }
  return p;
}

#define CHECK( c ) do { if( !(c) ) { fprintf( stderr, "case %lu: %s (line %d)\n", k, #c, __LINE__ ); return 1; } } while(0)

int
main( int argc, char ** argv ) {
  if( argc != 2 || !( f = fopen( argv[1], "rb" ) ) ) { fprintf( stderr, "usage: emit_host_check CASES\n" ); return 2; }
  char magic[8];
  if( fread( magic, 1, 8, f ) != 8 || memcmp( magic, "FDEMIT01", 8 ) ) return 2;
  ulong ncase = rd();
  for( ulong k=0; k<ncase; k++ ) {
    ulong fam = rd(), n = rd(), kc = rd();
    uint * keep = malloc( 4UL*kc + 1UL );
    for( ulong j=0; j<kc; j++ ) keep[j] = (uint)rd();
    void const ** a  = malloc( 8UL*n + 1UL );   /* msg / payload */
    void const ** sg = malloc( 8UL*n + 1UL );
    void const ** pb = malloc( 8UL*n + 1UL );
    ulong * sz   = malloc( 8UL*n + 1UL );
    ulong * doff = malloc( 8UL*(n + 1UL) );
    uchar * desc = NULL; ulong dtot = 0UL;
    doff[0] = 0UL;
    for( ulong i=0; i<n; i++ ) {
      if( !fam ) {
        sz[i] = rd(); pb[i] = rd_bytes( 32UL ); sg[i] = rd_bytes( 64UL ); a[i] = rd_bytes( sz[i] );
        CHECK( fd_ed25519_amd_emit_bound( sz[i] ) >= 96UL + sz[i] && !( fd_ed25519_amd_emit_bound( sz[i] ) & 127UL ) );
      } else {
        sz[i] = rd(); ulong F = rd();
        a[i] = rd_bytes( sz[i] );
        uchar * d = rd_bytes( F );
        desc = realloc( desc, dtot + F + 1UL );
        if( F ) memcpy( desc + dtot, d, F );
        free( d );
        dtot += F; doff[i+1] = dtot;
        if( F ) CHECK( fd_txn_amd_emit_bound( sz[i] ) >= ( ( sz[i] + 15UL ) & ~15UL ) + F + 2UL );
      }
    }
    if( fam && dtot ) { uchar * exact = malloc( dtot ); memcpy( exact, desc, dtot ); free( desc ); desc = exact; }
    ulong tot = rd();
    ulong * xoff = malloc( 8UL*(kc + 1UL) ); uint * xsz = malloc( 4UL*kc + 1UL );
    for( ulong j=0; j<=kc; j++ ) xoff[j] = rd();
    for( ulong j=0; j<kc; j++ ) xsz[j] = (uint)rd();
    uchar * img = rd_bytes( tot );

    for( int pass=0; pass<3; pass++ ) {   /* 0: exact capacity; 1: one byte short; 2: layout only */
      ulong cap = pass == 1 ? tot - 1UL : tot;
      if( pass == 1 && !tot ) continue;
      uchar * out  = pass == 2 ? NULL : malloc( cap + ( cap ? 0UL : 1UL ) );
      ulong * eoff = malloc( 8UL*(kc + 1UL) ); uint * esz = malloc( 4UL*kc + 1UL );
      if( out && cap ) memset( out, FILL, cap );
      memset( eoff, FILL, 8UL*(kc + 1UL) ); memset( esz, FILL, 4UL*kc );
      ulong got = fam ? fd_txn_amd_emit( kc, keep, (void const * const *)a, sz, doff, desc, out, cap, eoff, esz )
                      : fd_ed25519_amd_emit( kc, keep, (void const * const *)a, sz, (void const * const *)sg,
                                             (void const * const *)pb, out, cap, eoff, esz );
      if( pass == 1 ) {   /* ~0UL and nothing written */
        CHECK( got == ~0UL );
        for( ulong b=0; b<cap; b++ ) CHECK( out[b] == FILL );
        for( ulong b=0; b<8UL*(kc + 1UL); b++ ) CHECK( ((uchar *)eoff)[b] == FILL );
        for( ulong b=0; b<4UL*kc; b++ ) CHECK( ((uchar *)esz)[b] == FILL );
      } else {
        CHECK( got == tot );
        CHECK( !memcmp( eoff, xoff, 8UL*(kc + 1UL) ) );
        CHECK( !kc || !memcmp( esz, xsz, 4UL*kc ) );
        if( out && tot ) CHECK( !memcmp( out, img, tot ) );
      }
      free( out ); free( eoff ); free( esz );
    }

    for( ulong i=0; i<n; i++ ) { free( (void *)a[i] ); if( !fam ) { free( (void *)sg[i] ); free( (void *)pb[i] ); } }
    free( keep ); free( a ); free( sg ); free( pb ); free( sz ); free( doff ); free( desc ); free( xoff ); free( xsz ); free( img );
  }
  fclose( f );
  printf( "emit_host_check: %lu cases OK\n", ncase );
  return 0;
}
