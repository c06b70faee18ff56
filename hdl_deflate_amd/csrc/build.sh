#!/bin/bash
# Builds hdl_deflate_amd/lib/libhdlz.so for gfx950 (cross-compiles without a GPU).
# A/B builds: HDLZ_VARIANT=name HDLZ_DEFS="-DX=1 ..." build.sh  ->  lib/libhdlz_name.so (own object directory);
# select it at run time with HDLZ_LIB=hdl_deflate_amd/lib/libhdlz_name.so (see _lib.py, tools/ab.sh).
# HDLZ_ONLY="hdlz_compress hdlz_compress_small": only these sources are compiled with HDLZ_DEFS, the other objects are the main build's
# (which must exist).  `build.sh forced` builds lib/libhdlz_forced.so: the compress kernels with every fallback that this hardware never
# asks for FORCED (tests/test_gpu_forced_paths.py runs the compress parity tests on it).
if [ "${1:-}" = "forced" ]; then
  HDLZ_VARIANT=forced HDLZ_DEFS="-DHDLZ_HASH_FORCE_REORDER -DHDLZ_CHAIN_FORCE_SERIAL" \
    HDLZ_ONLY="hdlz_compress hdlz_compress_small hdlz_compress_stream hdlz_compress_chunk" exec "${BASH_SOURCE[0]}"
fi
# `build.sh keys` builds lib/libhdlz_keys.so: the one-tile kernel with the key-difference search instead of the bit-sliced one
# (tests/test_gpu_search_bits.py runs its blocks through both; tools/ab.sh times them against each other)
if [ "${1:-}" = "keys" ]; then
  HDLZ_VARIANT=keys HDLZ_DEFS="-DHDLZ_SEARCH_KEYS" HDLZ_ONLY="hdlz_compress" exec "${BASH_SOURCE[0]}"
fi
# `build.sh alllive` builds lib/libhdlz_alllive.so: the one-tile kernel that skips neither a constant bit plane nor the extension,
# parse and chain of a match-free tile (tests/test_gpu_dead_work.py runs its blocks through both forms; tools/ab.sh and
# tools/probe_dead_work.py time them against each other)
if [ "${1:-}" = "alllive" ]; then
  HDLZ_VARIANT=alllive HDLZ_DEFS="-DHDLZ_PLANES_ALL_LIVE -DHDLZ_NO_LITERAL_TILE" HDLZ_ONLY="hdlz_compress" exec "${BASH_SOURCE[0]}"
fi
# `build.sh dword` builds lib/libhdlz_dword.so: the one-tile kernel whose extension extracts the search's result bytes into registers
# and uses plain operands instead of the sub-dword (SDWA) forms (tests/test_gpu_wave_groups.py runs its blocks through both;
# tools/ab.sh times them against each other)
if [ "${1:-}" = "dword" ]; then
  HDLZ_VARIANT=dword HDLZ_DEFS="-DHDLZ_EXT_SDWA=0" HDLZ_ONLY="hdlz_compress" exec "${BASH_SOURCE[0]}"
fi
# `build.sh crcbank` builds lib/libhdlz_crcbank.so: the CRC-32 tile kernels with the bank-private table layout (hdlz_crc32.h;
# tools/probe_gzip.py times and counts it against the sliced tables)
if [ "${1:-}" = "crcbank" ]; then
  HDLZ_VARIANT=crcbank HDLZ_DEFS="-DHDLZ_CRC_BANK_PRIVATE" HDLZ_ONLY="hdlz_crc32 hdlz_unjoin" exec "${BASH_SOURCE[0]}"
fi
# `build.sh dbg` builds lib/libhdlz_dbg.so: the same kernels plus the host-only debug exports (hdlz_debug_par_offsets: where the control
# words of the two whole-GPU inflate chains lie in the caller's scratch; hdlz_debug_gunzip_crc).  tests/chain_verdict.py asks it for the
# layout (tests/test_gpu_chain_verdicts.py, tools/dev_any.py, tools/fuzz_any.py, tools/probe_gunzip.py)
if [ "${1:-}" = "dbg" ]; then
  HDLZ_VARIANT=dbg HDLZ_DEFS="-DHDLZ_DEBUG_EXPORTS" HDLZ_ONLY="hdlz_inflate_par hdlz_gunzip" exec "${BASH_SOURCE[0]}"
fi
set -euo pipefail
here="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
out="$here/../lib"
var="${HDLZ_VARIANT:-}"
objdir="$here/_obj${var:+_$var}"
lib="$out/libhdlz${var:+_$var}.so"
mkdir -p "$out" "$objdir"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function ${HDLZ_DEFS:-}"
srcs="hdlz_compress hdlz_compress_small hdlz_compress_stream hdlz_compress_chunk hdlz_inflate_tok hdlz_inflate_grp hdlz_inflate_par hdlz_inflate_any hdlz_inflate_dyn hdlz_checksum hdlz_compact hdlz_join hdlz_unjoin hdlz_crc32 hdlz_bgzf hdlz_bgzf_range hdlz_bgzf_stored hdlz_gunzip hdlz_gzip_members hdlz_zip hdlz_zip_write hdlz_seek hdlz_png hdlz_png_write hdlz_tiff hdlz_api"
only="${HDLZ_ONLY:-$srcs}"
pids=()
for f in $only; do
  src="$here/$f.hip"; obj="$objdir/$f.o"
  if [ ! -f "$obj" ] || [ "$src" -nt "$obj" ] || [ "${BASH_SOURCE[0]}" -nt "$obj" ] ||
     [ -n "$(find "$here" "$here/../../include" -maxdepth 1 -name '*.h' -newer "$obj" -print -quit)" ]; then
    ( "$HIPCC" $FLAGS -c "$src" -o "$obj" ) &
    pids+=($!)
  fi
done
rc=0
for p in "${pids[@]:-}"; do [ -n "$p" ] && { wait "$p" || rc=1; }; done
[ $rc -eq 0 ] || { echo "compile failed" >&2; exit 1; }
objs=""; for f in $srcs; do
  case " $only " in *" $f "*) objs="$objs $objdir/$f.o";; *) objs="$objs $here/_obj/$f.o";; esac
done
"$HIPCC" --offload-arch=gfx950 -shared -fPIC -o "$lib" $objs
echo "built $lib"
