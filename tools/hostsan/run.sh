#!/bin/bash
# Host-side AddressSanitizer + UndefinedBehaviorSanitizer runs of the library's host-only code
# (CPU, this container): the Merlin/STROBE transcript (both Keccak implementations; the batched
# record absorb against one append_message per record, at every block offset) and the
# Brakedown matgen (CSR invariants for SdigCode 1..6), and the stored files' image stager
# (pos_image.hpp: strided gather / scatter by mapping and by pread, the chunk-aligned row batches,
# the column-block partition), and the host-only half of the grouped ingest, scrub and repair of stored
# files (pos_rowgroup_plan.hpp, pos_repair_plan.hpp: the three planners over the fleets of the plan
# golden, the tables' ladder and copy, the column packing of scrub and repair with the rows that are not
# written and the listed columns of every image poisoned, empty groups and tables), and the grouped
# locate's own part of it (pos_locate_plan.hpp: the block with the locate records behind the repair's tables,
# the arenas' sizes, the counters).  GPU sanitizers are not available.
set -e -o pipefail
cd "$(dirname "$0")/../../lcpc_proof_of_storage_amd/csrc"
OUT=${TMPDIR:-/tmp}/lcpc_hostsan; mkdir -p "$OUT"
SAN="-O1 -g -std=c++20 -march=x86-64-v3 -fsanitize=address,undefined -fno-omit-frame-pointer -I."
g++ $SAN ../../tools/hostsan/transcript_san.cpp transcript.cpp -o "$OUT/transcript_san"
g++ $SAN -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include ../../tools/hostsan/matgen_san.cpp sdig_host.cpp transcript.cpp \
  -o "$OUT/matgen_san" -lpthread
g++ $SAN ../../tools/hostsan/pos_image_san.cpp -o "$OUT/pos_image_san" -lpthread
g++ $SAN -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include ../../tools/hostsan/pos_rowgroup_san.cpp -o "$OUT/pos_rowgroup_san" -lpthread
g++ $SAN -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include ../../tools/hostsan/pos_locate_san.cpp -o "$OUT/pos_locate_san" -lpthread
export ASAN_OPTIONS=detect_leaks=0 UBSAN_OPTIONS=halt_on_error=1
LCPC_KECCAK=scalar "$OUT/transcript_san"
LCPC_KECCAK=avx512 "$OUT/transcript_san"
"$OUT/matgen_san" | tail -1
"$OUT/pos_image_san"
"$OUT/pos_rowgroup_san"
"$OUT/pos_locate_san"
