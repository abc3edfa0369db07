/* tools/gen_budget_golden.c -- writes tests/golden/budget_vectors.bin, the
   expected compute budget records of the corpus of tests/_budget.py, from the
   REFERENCE's own fd_compute_budget_program_{init,parse,finalize}.

   The reference's header is included by include path and only when the
   fixture is regenerated; nothing of it is part of this repository, and the
   output holds data only (each payload and its 24-byte record).

     python tests/_budget.py dump /tmp/budget_in.bin
     gcc -O2 -std=gnu17 -I<reference>/src -Iinclude tools/gen_budget_golden.c -o /tmp/gen_budget_golden
     /tmp/gen_budget_golden /tmp/budget_in.bin tests/golden/budget_vectors.bin

   Input (tests/_budget.py: dump_input): "FDBUDGETINPUT01\0", u32 count, u32 0,
   then per case u32 payload size, u32 footprint, the payload, and the
   fd_txn_t that fd_txn_parse writes for it (footprint bytes; 0: rejected).
   Output: "FDBUDGETGOLDEN1\0", u32 count, u32 0, then per case u32 payload
   size, the payload, the fd_txn_amd_budget_t.

   The walk is the idiom of the reference's test_compute_budget_program.c,
   with the two rules include/fd_txn_amd.h adds: an instruction is looked at
   only if its program_id is below acct_addr_cnt, and a transaction with a
   rejected instruction has every field but the status zero. */
#include "ballet/pack/fd_compute_budget_program.h"   /* the reference's; brings its fd_txn.h */
#include "fd_txn_amd.h"                              /* ours: fd_txn_amd_budget_t (its Part 1 steps aside for the reference's) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static uint rd32( FILE * f ) { uint v; if( fread( &v, 4, 1, f ) != 1 ) { fprintf( stderr, "short input\n" ); exit( 1 ); } return v; }

static void
one( uchar const * p, fd_txn_t const * txn, fd_txn_amd_budget_t * out ) {
  memset( out, 0, sizeof(*out) );
  if( !txn ) { out->status = FD_TXN_AMD_BUDGET_NOPARSE; return; }
  fd_compute_budget_program_state_t st;
  fd_compute_budget_program_init( &st );
  for( ulong i=0UL; i<txn->instr_cnt; i++ ) {
    fd_txn_instr_t const * ix = txn->instr + i;
    if( ix->program_id >= txn->acct_addr_cnt ) continue;
    if( memcmp( p + txn->acct_addr_off + 32UL*ix->program_id, FD_COMPUTE_BUDGET_PROGRAM_ID, 32UL ) ) continue;
    if( !fd_compute_budget_program_parse( p + ix->data_off, ix->data_sz, &st ) ) { out->status = FD_TXN_AMD_BUDGET_INVALID; return; }
  }
  ulong rewards; uint compute;
  fd_compute_budget_program_finalize( &st, txn->instr_cnt, &rewards, &compute );
  out->rewards = rewards; out->compute = compute; out->heap_sz = st.heap_size; out->flags = st.flags;
  out->cb_instr_cnt = st.compute_budget_instr_cnt; out->status = FD_TXN_AMD_BUDGET_OK;
}

int
main( int argc, char ** argv ) {
  if( argc != 3 ) { fprintf( stderr, "usage: %s INPUT OUTPUT\n", argv[0] ); return 1; }
  FILE * in = fopen( argv[1], "rb" ), * out = fopen( argv[2], "wb" );
  char magic[16];
  if( !in || !out || fread( magic, 16, 1, in ) != 1 || memcmp( magic, "FDBUDGETINPUT01\0", 16 ) ) { fprintf( stderr, "bad files\n" ); return 1; }
  uint n = rd32( in ), zero = rd32( in );
  fwrite( "FDBUDGETGOLDEN1\0", 16, 1, out ); fwrite( &n, 4, 1, out ); fwrite( &zero, 4, 1, out );
  uchar * p = malloc( 65536UL + 8UL );
  ulong * d = malloc( 220512UL );   /* 8-aligned room for FD_TXN_AMD_FOOTPRINT_MAX */
  for( uint k=0U; k<n; k++ ) {
    uint sz = rd32( in ), fp = rd32( in );
    if( sz > 65536U || fp > 220502U || ( sz && fread( p, sz, 1, in ) != 1 ) || ( fp && fread( d, fp, 1, in ) != 1 ) ) { fprintf( stderr, "bad case %u\n", k ); return 1; }
    fd_txn_amd_budget_t r;
    one( p, fp ? (fd_txn_t const *)d : NULL, &r );
    fwrite( &sz, 4, 1, out ); if( sz ) fwrite( p, sz, 1, out ); fwrite( &r, sizeof(r), 1, out );
  }
  if( fclose( out ) ) return 1;
  printf( "%u cases\n", n );
  return 0;
}
