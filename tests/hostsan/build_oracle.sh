#!/bin/bash
# Builds $OUT/oracle_harness: the CPU oracle's three C files and tests/hostsan/oracle_harness.c under ASan + UBSan, with the host C
# compiler and the flags of oracle/Makefile (OpenMP kept). Plain C on the CPU: no device compiler, no device code. Called by
# build.sh (targets `oracle` and `all`); the same caching rule — an object is rebuilt when its source, the header or its command
# line changed — and the same last line, "compiled N".
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"
ROOT="$(cd "$HERE/../.." && pwd)"
OUT="${Q3_HOSTSAN_DIR:-$ROOT/build/hostsan}"
CC="${CC:-gcc}"
mkdir -p "$OUT"
# oracle/Makefile's flags (without -fPIC -shared: an executable) plus the sanitizers
OFLAGS="-O2 -ftree-vectorize -march=x86-64-v3 -ffp-contract=off -fno-fast-math -fopenmp -std=gnu11 -Wall -Wextra -Wno-unused-parameter -g -fsanitize=address,undefined -fno-sanitize-recover=undefined"
HDR="$ROOT/oracle/q3_oracle.h"
pids=(); objs=(); compiled=0
# compile <source> <object> <flags>
compile() {
  local src="$1" obj="$2" flags="$3"
  local cmd="$CC $flags -c $src -o $obj" stale=0
  objs+=("$obj")
  [ -f "$obj" ] && [ -f "$obj.cmd" ] && [ "$(cat "$obj.cmd")" = "$cmd" ] || stale=1
  for dep in "$src" "$HDR"; do [ "$dep" -nt "$obj" ] && stale=1; done
  if [ $stale = 1 ]; then
    rm -f "$obj.cmd"
    ( $cmd && echo "$cmd" > "$obj.cmd" ) &
    pids+=($!)
    compiled=$((compiled + 1))
  fi
}
for f in q3_oracle q3_oracle_spk q3_oracle_mimi; do
  compile "$ROOT/oracle/$f.c" "$OUT/o_$f.o" "$OFLAGS"
done
compile "$HERE/oracle_harness.c" "$OUT/oracle_harness.o" "$OFLAGS -I$ROOT/oracle"
fail=0
for p in "${pids[@]}"; do wait "$p" || fail=1; done
[ $fail = 0 ] || { echo "hostsan oracle build failed" >&2; exit 1; }
stale=0
[ -f "$OUT/oracle_harness" ] || stale=1
for o in "${objs[@]}"; do [ "$o" -nt "$OUT/oracle_harness" ] && stale=1; done
if [ $stale = 1 ]; then
  # (the runtimes linked in: the program needs no sanitizer library at load time)
  $CC -fopenmp -fsanitize=address,undefined -static-libasan -static-libubsan -o "$OUT/oracle_harness" "${objs[@]}" -lm
  echo "linked $OUT/oracle_harness"
fi
echo "compiled $compiled"
