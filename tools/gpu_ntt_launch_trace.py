"""The kernel launches of the NTT entry points at both sides of every routing threshold, as data: what
tests/golden/ntt_launch_trace.json records and tests/test_ntt_route.py holds the route (csrc/ntt/ntt_route.hpp) against.

    rocprofv3 --kernel-trace -d OUT0 -- python tools/gpu_ntt_launch_trace.py run 0 cases0.json
    rocprofv3 --kernel-trace -d OUT1 -- python tools/gpu_ntt_launch_trace.py run 1 cases1.json      (... one process per SETTINGS entry)
    python tools/gpu_ntt_launch_trace.py extract trace.json OUT0/.../*.db cases0.json OUT1/.../*.db cases1.json ...

`run K` executes the cases of SETTINGS[K] in one process on zero-filled device buffers (the launches do not depend on the
values) and writes what it ran to the cases file.  Setting 0 is the shipped library; the others are a tuning build
(-DSPPARK_TUNING in sppark_amd/lib_tuning, or where SPPARK_LIBDIR says; sppark_amd/build.py) with one SPPARK_NTT_* variable
each, which `run` sets itself before the library loads.  Every case runs once unrecorded first, so that every table is
cached; then once more with ONE tiny kernel of torch's (an in-place add on a one-element tensor) in front of each case.
`extract` reads the dispatch table as tools/gpu_msm_launch_trace.py does (its dispatch_rows) and cuts it at those marker
kernels: the last len(cases) dispatches of torch's are the markers, and a case is this library's kernels (names k_*)
between its marker and the next.  The table builders (BUILDERS) are dropped: where they run is a matter of what the cache
held.  Two runs of the same cases on the same device -- two commits -- must give the same trace.json.  A dispatch is
(index into "names", grid x, grid y, work-group size, LDS bytes), grids in work-items as the profiler reports them; a case
is CASE_COLUMNS + its dispatches."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gpu_msm_launch_trace import dispatch_rows          # noqa: E402

SETTINGS = ({}, {"SPPARK_NTT_R64_MIN": "99"}, {"SPPARK_NTT_R64_DIRECT": "12"}, {"SPPARK_NTT_COSET_FOLD": "0"}, {"SPPARK_NTT_LAT_SMAX": "0"})
BUILDERS = ("k_tables", "k_pass_table", "k_r64_table", "k_r64_cz", "k_pass_crow")
ELEM_BYTES = {"gl64": 8, "bb31": 4, "bls12_381": 32, "bn254": 32}
MODES = [(o, d, t) for o in range(4) for d in range(2) for t in range(2)]
BATCH_MODES = ((0, 0, 0), (1, 1, 1), (2, 0, 1), (3, 1, 0))
# kind: 0 one transform, 1 sppark_ntt_batch, 2 sppark_lde / sppark_lde_batch (lg = lg_domain, then order = lg_blowup);
# stride and offset (of the view into a 256-byte aligned buffer) in elements
CASE_COLUMNS = ["setting", "field", "kind", "lg", "order", "direction", "type", "batch", "stride", "offset"]


def cases(setting):
    out = []

    def case(field, kind, lg, order, direction=0, typ=0, batch=1, stride=0, offset=0):
        out.append([setting, field, kind, lg, order, direction, typ, batch, stride, offset])
    if setting == 0:
        for field, top in (("gl64", 24), ("bb31", 24), ("bls12_381", 20), ("bn254", 20)):
            for lg in range(1, top + 1):
                for m in MODES:
                    case(field, 0, lg, *m)
        for field in ("gl64", "bls12_381"):
            for lg in (3, 6, 7, 11, 12, 14):
                n = 1 << lg
                layouts = [(n, 0), (n + 4, 0)] + ([(n + 1, 0), (n, 1)] if field == "gl64" else [])
                for batch in (5, 300):
                    for stride, offset in layouts:
                        for m in BATCH_MODES:
                            case(field, 1, lg, *m, batch=batch, stride=stride, offset=offset)
            for lgd, lgb in ((3, 1), (8, 2), (11, 1), (12, 3), (16, 2), (12, 4), (0, 2)):
                for batch in (1, 3):
                    case(field, 2, lgd, lgb, batch=batch)
    elif setting in (1, 2, 3):
        for lg in (13, 18, 21):
            for m in MODES:
                case("gl64", 0, lg, *m)
    else:
        for lg in (10, 16):
            for m in MODES:
                case("bls12_381", 0, lg, *m)
    return out


def run(setting, meta_path):
    if setting:
        os.environ.setdefault("SPPARK_LIBDIR", "lib_tuning")
        os.environ.update(SETTINGS[setting])
    import torch
    from sppark_amd import ffi
    cs = cases(setting)
    need = 0
    for _s, field, kind, lg, order, _d, _t, batch, stride, offset in cs:
        n = 1 << (lg + order if kind == 2 else lg)
        need = max(need, (offset + (batch - 1) * (stride or n) + n) * ELEM_BYTES[field])
    buf = torch.zeros(need + 256, dtype=torch.uint8, device="cuda")
    base = (buf.data_ptr() + 255) & ~255
    mark = torch.zeros(1, dtype=torch.int32, device="cuda")
    libs = {f: ffi.load(f) for f in {c[1] for c in cs}}

    def one(c):
        _s, field, kind, lg, order, direction, typ, batch, stride, offset = c
        L = libs[field]
        p = base + offset * ELEM_BYTES[field]
        if kind == 0:
            ffi.check(L, L.sppark_ntt(0, p, lg, order, direction, typ, None))
        elif kind == 1:
            ffi.check(L, L.sppark_ntt_batch(0, p, lg, batch, stride, order, direction, typ, None))
        elif batch == 1:
            ffi.check(L, L.sppark_lde(0, p, lg, order, None, None))
        else:
            ffi.check(L, L.sppark_lde_batch(0, p, lg, order, batch, None, None))
    for c in cs:
        one(c)
    torch.cuda.synchronize()
    for c in cs:
        mark.add_(1)
        one(c)
    torch.cuda.synchronize()
    assert int(mark.item()) == len(cs)
    props = torch.cuda.get_device_properties(0)
    dev = dict(name=props.name, compute_units=props.multi_processor_count,
               max_grid_y=int(libs[cs[0][1]].sppark_ntt_batch_launch_cols(0, 16)))
    os.makedirs(os.path.dirname(os.path.abspath(meta_path)), exist_ok=True)
    with open(meta_path, "w") as f:
        json.dump(dict(device=dev, cases=cs), f)
    print("ran %d cases of setting %d -> %s" % (len(cs), setting, meta_path))


def extract(out_path, pairs):
    names, out, dev, cols = [], [], None, None
    for db_path, meta_path in pairs:
        meta = json.load(open(meta_path))
        assert dev in (None, meta["device"]), (dev, meta["device"])
        dev = meta["device"]
        cols, rows = dispatch_rows(db_path)
        assert len(cols) == 4, cols
        marks = [i for i, r in enumerate(rows) if "at::native" in r[0]][-len(meta["cases"]):]
        assert len(marks) == len(meta["cases"]) and len({rows[i][0] for i in marks}) == 1, (len(marks), len(meta["cases"]))
        marks.append(len(rows))
        for k, c in enumerate(meta["cases"]):
            disp = []
            for r in rows[marks[k] + 1:marks[k + 1]]:
                if not r[0].startswith("k_") or r[0].split("<")[0] in BUILDERS:
                    continue
                if r[0] not in names:
                    names.append(r[0])
                disp.append([names.index(r[0])] + list(r[1:]))
            out.append(list(c) + [disp])
    with open(out_path, "w") as f:
        json.dump(dict(device=dev, settings=SETTINGS, case_columns=CASE_COLUMNS + ["dispatches"], columns=["name"] + cols, names=names,
                       cases=out), f, separators=(",", ":"))
    print("%d cases, %d dispatches, %d kernels -> %s" % (len(out), sum(len(c[-1]) for c in out), len(names), out_path))


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "run":
        run(int(sys.argv[2]), sys.argv[3])
    elif len(sys.argv) >= 5 and sys.argv[1] == "extract" and len(sys.argv) % 2 == 1:
        extract(sys.argv[2], list(zip(sys.argv[3::2], sys.argv[4::2])))
    else:
        sys.exit(__doc__)
