"""Compares the HIP calls of two runs of one script, traced with
``rocprofv3 --hip-runtime-trace --kernel-trace -f json`` (the program after ``--``): the sequence
of kernel launches, memsets, event records and event waits with their stream and event
arguments (grid and block sizes for launches), and the kernel order of every queue.  Stream and
event handles differ from run to run, so each is named by the order of its first appearance.
Prints the counts and ``identical`` or the first difference.
usage: python tools/sweep_trace_compare.py A_results.json B_results.json"""
import json
import sys
from collections import Counter

CALLS = ("hipLaunchKernel", "hipExtLaunchKernel", "hipModuleLaunchKernel", "hipExtModuleLaunchKernel",
         "hipMemsetAsync", "hipEventRecord", "hipStreamWaitEvent", "hipStreamIsCapturing",
         "hipEventCreateWithFlags", "hipStreamCreateWithFlags")


def load(path):
    tool = json.load(open(path))["rocprofiler-sdk-tool"][0]
    names = {s["kind"]: s["operations"] for s in tool["strings"]["buffer_records"]}
    kind_name = {i: s["kind"] for i, s in enumerate(tool["strings"]["buffer_records"])}
    seq, handles = [], {}

    def alias(kind, value):   # handles by order of first appearance; stream 0 is the null stream
        if value in ("0", "0x0", 0):
            return kind + "0"
        return handles.setdefault((kind, value), f"{kind}{sum(k == kind for k, _ in handles) + 1}")

    for r in sorted(tool["buffer_records"]["hip_api"], key=lambda r: r["start_timestamp"]):
        fn = names[kind_name[r["kind"]]][r["operation"]]
        if fn not in CALLS:
            continue
        item = [fn]
        for a in r.get("args", []):
            if a["name"] in ("stream", "hStream"):
                item.append(alias("s", a["value"]))
            elif a["name"] == "event" and "Create" not in fn:
                item.append(alias("e", a["value"]))
            elif a["name"] in ("numBlocks", "dimBlocks", "sharedMemBytes", "value", "sizeBytes"):
                item.append(a["value"])
        seq.append(tuple(item))
    syms = {k["kernel_id"]: k["formatted_kernel_name"] for k in tool["kernel_symbols"]}
    queues = {}
    for d in sorted(tool["buffer_records"]["kernel_dispatch"], key=lambda d: d["dispatch_info"]["dispatch_id"]):
        i = d["dispatch_info"]
        queues.setdefault(i["queue_id"]["handle"], []).append(syms.get(i["kernel_id"], i["kernel_id"]))
    # queues by order of first dispatch
    return seq, list(queues.values())


def first_difference(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return f"first difference at {i}: {x} | {y}"
    return "identical" if len(a) == len(b) else f"lengths differ: {len(a)} | {len(b)}"


def main():
    (sa, qa), (sb, qb) = load(sys.argv[1]), load(sys.argv[2])
    ca, cb = Counter(x[0] for x in sa), Counter(x[0] for x in sb)
    for fn in CALLS:
        if ca[fn] or cb[fn]:
            print(f"  {fn}: {ca[fn]} | {cb[fn]}")
    print(f"  streams named: {len({t for x in sa for t in x[1:] if str(t)[0] == 's'})} | "
          f"{len({t for x in sb for t in x[1:] if str(t)[0] == 's'})}; events named: "
          f"{len({t for x in sa for t in x[1:] if str(t)[0] == 'e'})} | "
          f"{len({t for x in sb for t in x[1:] if str(t)[0] == 'e'})}")
    print("  call sequence with stream / event arguments:", first_difference(sa, sb))
    print(f"  queues with kernels: {len(qa)} | {len(qb)}; dispatches: {sum(map(len, qa))} | {sum(map(len, qb))}")
    for i, (x, y) in enumerate(zip(qa, qb)):
        print(f"  kernel order of queue {i} ({len(x)} | {len(y)} kernels):", first_difference(x, y))
    same = first_difference(sa, sb) == "identical" and len(qa) == len(qb) and all(x == y for x, y in zip(qa, qb))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
