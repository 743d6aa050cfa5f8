#!/bin/bash
# Shadow-hit lookups at 16 callers, three ways in one session, alternating: the library of the commit before measured load
# (<parent dir>/librio_gp.so, built from that commit by the caller), the library of this tree with tracking off, and with
# tracking on.  tools/measure_ops.py has no leg with concurrent callers, hence a program for this: tools/load_tracking_host_probe.c.
# Usage: tools/load_tracking_host_ab.sh <parent dir> [rounds] > out.jsonl      (rounds: a multiple of 3 balances the order)
set -u -o pipefail
PARENT=${1:?usage: load_tracking_host_ab.sh PARENT_DIR [ROUNDS]}
ROUNDS=${2:-3}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
PARENT=$(cd "$PARENT" && pwd) || exit 1
[ -f "$PARENT/librio_gp.so" ] || { echo "no librio_gp.so in $PARENT" >&2; exit 1; }
[ -f "$ROOT/rio-rs_amd/librio_gp.so" ] || { echo "no librio_gp.so in $ROOT/rio-rs_amd: build first" >&2; exit 1; }
TMP=$(mktemp -d) || exit 1
trap 'rm -rf "$TMP"' EXIT
gcc -O2 -std=c99 -pthread -DNO_LOAD_TRACKING -I "$ROOT/include" "$ROOT/tools/load_tracking_host_probe.c" -o "$TMP/probe_parent" \
    -L "$PARENT" -lrio_gp -Wl,-rpath,"$PARENT" -Wl,-rpath,/opt/rocm/lib || exit 1
gcc -O2 -std=c99 -pthread -I "$ROOT/include" "$ROOT/tools/load_tracking_host_probe.c" -o "$TMP/probe_new" \
    -L "$ROOT/rio-rs_amd" -lrio_gp -Wl,-rpath,"$ROOT/rio-rs_amd" -Wl,-rpath,/opt/rocm/lib || exit 1
run_one() {
    case $1 in
        0) timeout -k 10 120 "$TMP/probe_parent" parent 0 20000 2000000 5 16 ;;
        1) timeout -k 10 120 "$TMP/probe_new" tracking_off 0 20000 2000000 5 16 ;;
        2) timeout -k 10 120 "$TMP/probe_new" tracking_on 1 20000 2000000 5 16 ;;
    esac
}
for r in $(seq 1 "$ROUNDS"); do   # the order rotates from round to round: no build always runs behind the same one
    for k in 0 1 2; do
        run_one $(( (k + r - 1) % 3 )) || exit $?
    done
done
