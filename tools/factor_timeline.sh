# timeline of ONE refactorisation (last of a short bench run): start us, end us, duration us, queue, kernel class, workgroups; then the
# span from the first to the last tile kernel, the time in launches of <= 1131 workgroups, and the time during which two or more tile
# kernels run (the subdomain groups' chains, DOTMI_TILE_GROUPS)
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd /tmp && export TMPDIR=/tmp
rm -rf /tmp/prof; rocprofv3 --kernel-trace --output-format csv -d /tmp/prof -- python "$ROOT/bench.py" --steps 4 --warmup 2 --no-cpu-baseline --extra-workloads none "$@" > /tmp/b.log 2>&1
f=$(find /tmp/prof -name "*kernel_trace.csv" | head -1)
python - "$f" <<'PY'
import csv,sys,collections
rows=list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r:int(r['Start_Timestamp']))
def cls(n):
    if 'tile_gemm' in n: return 'tgemm'
    if 'tile_task' in n: return 'tile'
    if 'clear_tiles' in n: return 'clear'
    if 'elem_hessian' in n: return 'elemH'
    if 'assemble' in n: return 'assemble'
    if 'clear_segments' in n: return 'clear'
    if 'dense_fill' in n: return 'fill'
    if 'pad_identity' in n: return 'pad'
    return None
runs=[];cur=[]
for r in rows:
    c=cls(r['Kernel_Name'])
    if c: cur.append(r)
    else:
        if len(cur)>20: runs.append(cur)
        cur=[]
if len(cur)>20: runs.append(cur)
fr=[r for r in runs if any(cls(k['Kernel_Name']) in ('tile','tgemm') for k in r)]
run=fr[-1]
t0=int(run[0]['Start_Timestamp'])
qs={}
tiles=[r for r in run if cls(r['Kernel_Name'])=='tile']
for r in run:
    q=r['Queue_Id']; qs.setdefault(q,len(qs))
    wg=int(r['Grid_Size_X'])*int(r['Grid_Size_Y'])*int(r['Grid_Size_Z'])//max(1,int(r['Workgroup_Size_X'])*int(r['Workgroup_Size_Y'])*int(r['Workgroup_Size_Z']))
    print("%8.1f %8.1f %7.1f q%d %-8s wg %5d"%((int(r['Start_Timestamp'])-t0)/1e3,(int(r['End_Timestamp'])-t0)/1e3,(int(r['End_Timestamp'])-int(r['Start_Timestamp']))/1e3,qs[q],cls(r['Kernel_Name']),wg))
print("wall", (max(int(r['End_Timestamp']) for r in run)-t0)/1e3)
if tiles:
    a=min(int(r['Start_Timestamp']) for r in tiles); b=max(int(r['End_Timestamp']) for r in tiles)
    print("factorisation: first tile kernel starts %.1f us, last ends %.1f us, span %.1f us, %d launches"%((a-t0)/1e3,(b-t0)/1e3,(b-a)/1e3,len(tiles)))
    def wgs(r): return int(r['Grid_Size_X'])//max(1,int(r['Workgroup_Size_X']))
    small=sum(int(r['End_Timestamp'])-int(r['Start_Timestamp']) for r in tiles if wgs(r)<=1131)
    print("time in tile launches of <= 1131 workgroups: %.1f us (%.1f %% of the span), %d launches"%(small/1e3,100.0*small/(b-a),sum(1 for r in tiles if wgs(r)<=1131)))
    # overlap: time during which >= 2 tile kernels run
    ev=[]
    for r in tiles: ev+= [(int(r['Start_Timestamp']),1),(int(r['End_Timestamp']),-1)]
    ev.sort(); n=0; last=0; ov=0
    for t,d in ev:
        if n>=2: ov+=t-last
        n+=d; last=t
    print("time with two or more tile kernels running: %.1f us"%(ov/1e3))
PY
