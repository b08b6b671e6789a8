#!/bin/bash
# isa_diff.sh REV — is the gfx950 device code of the working tree the same as REV's?
# Compiles every csrc/*.hip (and the second builds: recording, evaluation) of REV, from a temporary git worktree,
# and of the working tree to device assembly with the Makefile's flags, and diffs them file by
# file. Only the translation-unit id __hip_cuid_<hex> (a hash of the source text) is erased.
# Prints `identical` or the first lines of the diff per file, and for a file that differs one line
# per kernel with both sides' instruction-line count and register / spill / LDS / scratch metadata;
# exit status 1 if any file differs.
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
    if grep -q DADMM_ROLES_EVAL "$1/$SUB/dadmm_fused_roles.hip"; then   # the evaluation kernels' build
        echo "dadmm_fused_roles_eval $1/$SUB/dadmm_fused_roles.hip -DDADMM_ROLES_EVAL=1"
    fi
    if grep -q DADMM_STREAM_EVAL "$1/$SUB/dadmm_stream.hip"; then   # the streamed evaluation kernels' build
        echo "dadmm_stream_eval $1/$SUB/dadmm_stream.hip -DDADMM_STREAM_EVAL=1"
    fi
}
mkdir "$TMP/a" "$TMP/b"
{ units "$TMP/old" | sed "s|^|$TMP/a |"; units "$ROOT" | sed "s|^|$TMP/b |"; } |
    xargs -P "${JOBS:-16}" -L 1 bash -c \
        '$0 $4 -x hip --cuda-device-only -S "$3" -o "$1/$2.s" 2>"$1/$2.err" || { cat "$1/$2.err"; rm -f "$1/$2.s"; }' "$FLAGS"
norm() { sed -E 's/__hip_cuid_[0-9a-f]+/__hip_cuid/g' "$1"; }
# "kernel insts vgpr sgpr vgpr_spill sgpr_spill lds scratch" per kernel of the assembly file $1:
# the instruction lines between the kernel's label and its .Lfunc_end, and the code object
# metadata's register, spill, LDS (.group_segment_fixed_size) and scratch
# (.private_segment_fixed_size) values. Lines are counted, not read.
kstats() {
    awk '
        function flush() {
            if (name != "")
                print name, n[name] + 0, v["vgpr_count"], v["sgpr_count"], v["vgpr_spill_count"],
                      v["sgpr_spill_count"], v["group_segment_fixed_size"], v["private_segment_fixed_size"]
            name = ""; split("", v)
        }
        /^[A-Za-z_][A-Za-z0-9_$.]*:/ { cur = $1; sub(/:.*/, "", cur) }
        /^\.Lfunc_end/ { cur = "" }
        cur != "" && /^\t[a-z]/ { n[cur]++ }
        /^  - \./ { flush() }
        /^ +(- )?\.name: / && !/^ {5}/ { name = $NF }
        /^ +(- )?\.[a-z_]+: +[0-9]+$/ && !/^ {5}/ { k = $(NF - 1); sub(/^\./, "", k); sub(/:$/, "", k); v[k] = $NF }
        END { flush() }' "$1" | sort
}
rc=0
for n in $(units "$ROOT" | cut -d' ' -f1); do
    if ! units "$TMP/old" | cut -d' ' -f1 | grep -qx "$n" && [ -f "$TMP/b/$n.s" ]; then
        echo "$n: new unit (not in $REV)"; kstats "$TMP/b/$n.s" | sed 's/^/  /'; continue
    fi
    if [ ! -f "$TMP/a/$n.s" ] || [ ! -f "$TMP/b/$n.s" ]; then rc=1; echo "$n: not compiled on both sides"; continue; fi
    if d=$(diff <(norm "$TMP/a/$n.s") <(norm "$TMP/b/$n.s")); then echo "$n: identical"
    else
        rc=1; echo "$n: DIFFERS ($(wc -l <<<"$d") diff lines)"; head -n 12 <<<"$d"
        echo "  per kernel, REV -> working tree: insts vgpr sgpr vgpr_spill sgpr_spill lds scratch"
        join -a 1 -a 2 -e - -o 0,1.2,2.2,1.3,2.3,1.4,2.4,1.5,2.5,1.6,2.6,1.7,2.7,1.8,2.8 \
            <(kstats "$TMP/a/$n.s") <(kstats "$TMP/b/$n.s") |
            awk '{ printf "  %s:", $1; for (i = 2; i < NF; i += 2) printf " %s->%s", $i, $(i + 1); print "" }' |
            { if command -v c++filt >/dev/null; then c++filt; else cat; fi; }
    fi
done
exit $rc
