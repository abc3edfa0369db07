/* oracle/txn_limits_check.c -- TEST INFRASTRUCTURE ONLY (CPU, never on a GPU box).
 *
 * Memory-safety check of the transaction-parser restatement
 * (oracle/fd_txn_oracle.c) on payloads of any size the parser accepts.
 * `make -C oracle sanitize` compiles this file and the oracle's sources
 * together with -fsanitize=address,undefined into one stand-alone program
 * and runs it on the directed grammar-limit payloads (tests/_txn.py:
 * limit_cases, written out by tools/gen_txn_limits.py).
 *
 *   txn_limits_check <packed payload file>
 *
 * packed file (little endian): u32 count, count x { u32 sz, payload[sz] }.
 *
 * Every payload is copied into a heap block of exactly its size and parsed
 * into a heap block of exactly oracle_txn_desc_max() bytes, so a read past
 * the payload or a store past the descriptor capacity is a sanitizer
 * report; oracle_txn_parse_fail_line runs on the same copy.  Exit status 0
 * and the summary line mean no report.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

typedef unsigned char uchar;
typedef unsigned long ulong;

ulong oracle_txn_desc_max( void );
ulong oracle_txn_parse( uchar const * payload, ulong payload_sz, void * out_buf, void * counters_opt );
ulong oracle_txn_parse_fail_line( uchar const * payload, ulong payload_sz );

static int
rd32( FILE * f, uint32_t * v ) {
  uchar b[4];
  if( fread( b, 1, 4, f ) != 4 ) return 0;
  *v = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
  return 1;
}

int
main( int argc, char ** argv ) {
  if( argc != 2 ) { fprintf( stderr, "usage: %s <packed payload file>\n", argv[0] ); return 2; }
  FILE * f = fopen( argv[1], "rb" );
  if( !f ) { perror( argv[1] ); return 2; }
  uint32_t cnt;
  if( !rd32( f, &cnt ) ) { fprintf( stderr, "short file\n" ); return 2; }
  ulong cap = oracle_txn_desc_max();
  ulong ok = 0UL, rej = 0UL, fp_max = 0UL, sz_max = 0UL;
  for( uint32_t k=0U; k<cnt; k++ ) {
    uint32_t sz;
    if( !rd32( f, &sz ) ) { fprintf( stderr, "short file at payload %u\n", k ); return 2; }
    uchar * p = (uchar *)malloc( sz ? sz : 1U );
    uchar * out = (uchar *)malloc( cap );
    if( !p || !out || fread( p, 1, sz, f ) != sz ) { fprintf( stderr, "payload %u unreadable\n", k ); return 2; }
    ulong fp = oracle_txn_parse( sz ? p : NULL, sz, out, NULL );
    ulong line = oracle_txn_parse_fail_line( sz ? p : NULL, sz );
    if( fp > cap || (fp != 0UL) != (line == 0UL) ) {
      fprintf( stderr, "payload %u: footprint %lu (capacity %lu), line %lu\n", k, fp, cap, line );
      return 1;
    }
    if( fp ) ok++; else rej++;
    if( fp > fp_max ) fp_max = fp;
    if( sz > sz_max ) sz_max = sz;
    free( out ); free( p );
  }
  fclose( f );
  printf( "txn_limits_check: %u payloads (largest %lu B), %lu accepted, %lu rejected, largest footprint %lu of capacity %lu: clean\n",
          cnt, sz_max, ok, rej, fp_max, cap );
  return 0;
}
