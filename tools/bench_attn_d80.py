"""the 32x32-level self-attention (head_dim 80, 1024 queries per frame, three sources) with prescaled q, as the UNet dispatches it
(the generic body with the accumulator-folded reference).  Run under rocprofv3 --pmc for its SQ counters; a kernel variant is compared
as a second build of the library (tools/ab.sh UNIVST_LIB=a,b)."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_attn import run
run(8, 80, 1024, 16, 3, iters=2, prescaled=True)
