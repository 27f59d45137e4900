cd "$(dirname "$0")/../.." && export TMPDIR=/tmp; O=${O:-build/r5d}; mkdir -p $O
for w in "" "--emulate-wire 64" ; do for f in 16 32; do
python bench.py --full --frames $f --emulate-rank 1/8 $w --steps 20 --warmup 3 --no-cpu-baseline > $O/emu_f${f}_$(echo $w | tr -d ' -').json 2>> $O/err
done; done
O=$O python - <<'PY'
import json,glob,os
for f in sorted(glob.glob(os.environ["O"] + "/emu_*.json")):
    try:
        d=json.loads(open(f).read().strip().splitlines()[-1]); c=d["roofline"]["classes"]
        print(f, d["ms_per_step"], d["config"].get("modelled_wire_ms_per_step"), {k:v["ms_per_step"] for k,v in c.items() if v["ms_per_step"]>0.15})
    except Exception as e: print(f, "ERR", e)
PY
rocprofv3 --kernel-trace --output-format csv -d $O/trace -- python bench.py --emulate-rank 1/8 --steps 10 --warmup 2 --no-cpu-baseline --no-profile > $O/emu_trace.json 2>> $O/err
python tools/step_shapes.py $O/trace 13 > $O/shapes_emu.txt 2>&1; find $O/trace -type f -size +512k -delete
head -60 $O/shapes_emu.txt
tail -3 $O/err
