# LDS counters of the SGBM kernels (tooling): per library in $LIBS (tree = the in-tree library, any
# other name v = exp/libfvo_v.so through FVO_LIB) two counters-only rocprofv3 --pmc passes of
# tools/bench_sgbm.py -- LDS-array cycles and bank-conflict cycles, then LDS instructions and their
# issue cycles -- each with GRBM_GUI_ACTIVE; CSVs under $OUT/<lib>/<pass>/ ($OUT relative to the
# repository root, default prof_sglds) and a per-kernel summary $OUT/<lib>_<pass>.csv.
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
O=$R/${OUT:-prof_sglds}
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
rocprofv3 -L 2>/dev/null | grep -o 'SQ_[A-Z_]*LDS[A-Z_]*' | sort -u > $O/counters.txt
for v in ${LIBS:-tree}; do
  lib=""; [ "$v" = tree ] || lib=$R/exp/libfvo_$v.so
  n=0
  for set in "SQ_LDS_IDX_ACTIVE SQ_LDS_BANK_CONFLICT SQ_LDS_ADDR_CONFLICT GRBM_GUI_ACTIVE" \
             "SQ_INSTS_LDS SQ_ACTIVE_INST_LDS SQ_WAVES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE"; do
    n=$((n + 1))
    rm -rf /tmp/sglds_${v}_$n
    FVO_LIB=$lib timeout -s KILL 120 rocprofv3 --pmc $set --kernel-include-regex 'k_sg_' --output-format csv \
      -d /tmp/sglds_${v}_$n -o pmc -- python3 $R/tools/bench_sgbm.py ${BENCH_ARGS:-} > $O/${v}_$n.out 2>&1 || { tail -20 $O/${v}_$n.out; exit 1; }
    mkdir -p $O/$v/$n && find /tmp/sglds_${v}_$n -name "*counter_collection.csv" -exec cp {} $O/$v/$n/ \;
    python3 $R/profiles/summarize_pmc.py $O/$v/$n $O/${v}_$n.csv 600p k_sg_ || exit 1
  done
done
exit 0
