#!/bin/bash
# isa_diff.sh REV — is the gfx950 device code of the working tree the same as REV's?
# Compiles every csrc/*.hip (and the two recording builds) of REV, from a temporary git worktree,
# and of the working tree to device assembly with the Makefile's flags, and diffs them file by
# file. Only the translation-unit id __hip_cuid_<hex> (a hash of the source text) is erased.
# Prints `identical` or the first lines of the diff per file; exit status 1 if any file differs.
set -euo pipefail
REV=${1:?usage: isa_diff.sh REV}
ROOT=$(git -C "$(dirname "$0")" rev-parse --show-toplevel)
SUB=hyperparameter-gnn_unfolded-d-admm-main_amd/csrc
TMP=$(mktemp -d)
trap 'git -C "$ROOT" worktree remove --force "$TMP/old" 2>/dev/null; rm -rf "$TMP"' EXIT
git -C "$ROOT" worktree add --detach "$TMP/old" "$REV" >/dev/null
FLAGS=$(make -s -C "$ROOT/$SUB" -f Makefile -f <(echo 'isa-flags:; @echo $(HIPCC) $(FLAGS)') isa-flags)
units() {   # "name source extra-flag" per compile unit of the tree $1
    for f in "$1/$SUB"/*.hip; do echo "$(basename "$f" .hip) $f"; done
    echo "dadmm_fused_rec $1/$SUB/dadmm_fused.hip -DDADMM_FUSED_REC=1"
    echo "dadmm_split_rec $1/$SUB/dadmm_split.hip -DDADMM_SPLIT_REC=1"
}
mkdir "$TMP/a" "$TMP/b"
{ units "$TMP/old" | sed "s|^|$TMP/a |"; units "$ROOT" | sed "s|^|$TMP/b |"; } |
    xargs -P "${JOBS:-16}" -L 1 bash -c \
        '$0 $4 -x hip --cuda-device-only -S "$3" -o "$1/$2.s" 2>"$1/$2.err" || { cat "$1/$2.err"; rm -f "$1/$2.s"; }' "$FLAGS"
norm() { sed -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid/g' "$1"; }
rc=0
for n in $(units "$ROOT" | cut -d' ' -f1); do
    if [ ! -f "$TMP/a/$n.s" ] || [ ! -f "$TMP/b/$n.s" ]; then rc=1; echo "$n: not compiled on both sides"; continue; fi
    if d=$(diff <(norm "$TMP/a/$n.s") <(norm "$TMP/b/$n.s")); then echo "$n: identical"
    else rc=1; echo "$n: DIFFERS ($(wc -l <<<"$d") diff lines)"; head -n 12 <<<"$d"; fi
done
exit $rc
