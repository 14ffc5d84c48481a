"""The ordered list of kernel launches of one solve per driver branch of pph_solve.hip, for comparing two builds of the
library launch for launch (a restructuring of the host drivers must leave every list as it was).

    python tools/launch_sequence.py CASE            runs one case (the program to put behind `rocprofv3 --kernel-trace ... --`)
    python tools/launch_sequence.py --list          the case names
    python tools/launch_sequence.py --all OUTDIR    every case once, each in a process of its own under
                                                    `rocprofv3 --kernel-trace` (no counters, no other tracing); prints per case
                                                    the launch count and the SHA-256 of the ordered list of
                                                    (kernel name, grid, workgroup size), and keeps the lists in OUTDIR/CASE.txt
    python tools/launch_sequence.py --digest CSV    the same two figures for one kernel-trace CSV

The library is the one PERPHIL_HIP_LIB names (default: the tree's own), so two builds are compared by running `--all` twice
(profiles/solve_refactor_launch_sequences.txt)."""
import csv
import glob
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _picard(**kw):
    # (no inner_reduction: with inner_max_it 3 every block solve runs its three iterations, all halves of the loop body)
    d = dict(picard=1, inner_ksp="cg", inner_pc="mg", inner_rtol=1e-10, inner_reduction=0.0, mg_smooth=1, picard_rtol=1e-8)
    d.update(kw)
    return d


# name -> (mesh, context options, solver configuration)
HEX16, QUAD32, QUAD16 = ("hex", 16, 16, 16), ("quad", 32, 32, 0), ("quad", 16, 16, 0)
CASES = {
    "picard_mg_norm0": (HEX16, {}, _picard(inner_norm=0, inner_max_it=3)),
    "picard_mg_norm1": (HEX16, {}, _picard(inner_norm=1, inner_max_it=3)),
    "picard_mg_norm2": (HEX16, {}, _picard(inner_norm=2, inner_max_it=3)),
    "picard_mg_norm1_graphs2": (HEX16, {"use_graphs": 2}, _picard(inner_norm=1, inner_max_it=3)),
    "picard_mg_norm2_graphs2": (HEX16, {"use_graphs": 2}, _picard(inner_norm=2, inner_max_it=3)),
    "picard_jacobi": (HEX16, {}, _picard(inner_pc="jacobi", inner_norm=0, inner_max_it=50000, inner_reduction=0.0)),
    "picard_gmres": (HEX16, {}, _picard(inner_ksp="gmres", inner_pc="jacobi", inner_max_it=50000, inner_reduction=0.0)),
    "mono_cg_block2": (QUAD32, {}, dict(ksp="cg", pc="block2", rtol=1e-10)),
    "mono_cg_jacobi": (QUAD32, {}, dict(ksp="cg", pc="jacobi", rtol=1e-10)),
    "mono_cg_cmg": (QUAD32, {}, dict(ksp="cg", pc="cmg", rtol=1e-10)),
    "gmres_fieldsplit_mg": (HEX16, {}, dict(ksp="gmres", pc="fieldsplit", inner_ksp="cg", inner_pc="mg", inner_rtol=1e-10)),
    "fieldsplit_lu_blocks": (QUAD16, {}, dict(ksp="gmres", pc="fieldsplit", inner_ksp="cg", inner_pc="mg", inner_rtol=1e-12,
                                              inner_exact=1)),
    "transient_two_steps": (HEX16, {}, _picard(inner_norm=1, inner_max_it=50000, inner_reduction=1e-1)),
}


def run_case(name):
    import numpy as np

    from oracle import dpp_oracle as o
    from perphil_amd import _ffi as f

    (kind, nx, ny, nz), opts, kw = CASES[name]
    dim, cell = (3, o.CELL_HEX) if kind == "hex" else (2, o.CELL_QUAD)
    P = o.Params(k1=1.0, k2=0.01, beta=1.0, mu=1.0)
    om = o.build_mesh(dim, cell, nx, ny, nz)
    b = o.boundary_nodes(om)
    e1, e2 = o.exact_pressures(om.coords, P)
    c = f.SolverCfg()
    c.ksp_type, c.pc_type, c.restart, c.max_it, c.rtol, c.atol = f.KSP_GMRES, f.PC_NONE, 30, 50000, 1e-8, 1e-12
    c.inner_ksp_type, c.inner_pc_type, c.inner_max_it, c.inner_rtol, c.inner_atol = f.KSP_CG, f.PC_JACOBI, 50000, 1e-12, 1e-300
    c.picard, c.picard_rtol, c.picard_atol, c.picard_max_it, c.mg_smooth = 0, 1e-8, 1e-12, 100, 2
    ksp = {"cg": f.KSP_CG, "gmres": f.KSP_GMRES}
    pc = {"jacobi": f.PC_JACOBI, "mg": f.PC_MG, "block2": f.PC_BLOCK2, "cmg": f.PC_CMG, "fieldsplit": f.PC_FIELDSPLIT}
    for k, v in kw.items():
        if k in ("ksp", "inner_ksp"):
            setattr(c, k + "_type", ksp[v])
        elif k in ("pc", "inner_pc"):
            setattr(c, k + "_type", pc[v])
        else:
            setattr(c, k, v)
    with f.Context(0) as ctx:
        for k, v in opts.items():
            ctx.set_option(k, v)
        ctx.mesh_build(dim, cell, nx, ny, nz)
        ctx.set_dirichlet(0, b, e1[b])
        ctx.set_dirichlet(1, b, e2[b])
        if name.startswith("transient"):
            ctx.transient_begin(P.k1, P.k2, P.beta, P.mu, (1.0, 1.0), 1.0, 0.1, monolithic=False)
            p = np.zeros(2 * ctx.n)
            done, infos, _ = ctx.transient_steps(c, p, 2)
            print(f"{name}: {done} steps, sweeps {[i.iterations for i in infos[:done]]}, inner {[i.inner_iterations for i in infos[:done]]}")
            return
        ctx.assemble(P.k1, P.k2, P.beta, P.mu, monolithic=not c.picard)
        x, info, _ = ctx.solve(c, raise_on_diverged=False)
        print(f"{name}: iterations {info.iterations}, inner {info.inner_iterations}, converged {info.converged}, "
              f"inner_failed {info.inner_failed}, resnorm {info.resnorm:.17g}, sha256(x) {hashlib.sha256(x.tobytes()).hexdigest()[:16]}")


def launches(path):
    """[(kernel name, grid, workgroup size)] of a rocprofv3 kernel-trace CSV, in the order of dispatch"""
    with open(path, newline="") as fh:
        rows = list(csv.DictReader(fh))
    rows.sort(key=lambda r: (int(r["Dispatch_Id"]) if r.get("Dispatch_Id") else 0, int(r["Start_Timestamp"])))
    return [(r["Kernel_Name"], tuple(int(r["Grid_Size_" + a]) for a in "XYZ"), tuple(int(r["Workgroup_Size_" + a]) for a in "XYZ"))
            for r in rows]


def digest(seq):
    text = "".join(f"{k} {g[0]}x{g[1]}x{g[2]} {w[0]}x{w[1]}x{w[2]}\n" for k, g, w in seq)
    return len(seq), hashlib.sha256(text.encode()).hexdigest(), text


def run_all(out):
    os.makedirs(out, exist_ok=True)
    for name in CASES:
        d = os.path.join(out, "trace_" + name)
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "kt", "--",
                            sys.executable, os.path.abspath(__file__), name], capture_output=True, text=True, timeout=300)
        if r.returncode != 0:   # nothing more is started on the device after a failure
            sys.exit(f"{name}: exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        found = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if len(found) != 1:
            sys.exit(f"{name}: {len(found)} kernel-trace files under {d}")
        count, sha, text = digest(launches(found[0]))
        with open(os.path.join(out, name + ".txt"), "w") as fh:
            fh.write(text)
        solve_line = [ln for ln in r.stdout.splitlines() if ln.startswith(name + ":")]
        print(f"{name:26s} launches {count:6d}  sha256 {sha}  | {solve_line[-1] if solve_line else ''}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "--list":
        print("\n".join(CASES))
    elif len(sys.argv) == 3 and sys.argv[1] == "--all":
        run_all(sys.argv[2])
    elif len(sys.argv) == 3 and sys.argv[1] == "--digest":
        count, sha, _ = digest(launches(sys.argv[2]))
        print(count, sha)
    elif len(sys.argv) == 2 and sys.argv[1] in CASES:
        run_case(sys.argv[1])
    else:
        sys.exit(__doc__)
