"""Longer session walks by hand: random call sequences over every entry point on 24 live sequences, each call held to the
model of tests/session_model.py.  usage: fuzz_session.py [n_walks] [seed] [n_ops] [shape]
tests/test_gpu_session_walk.py runs a few seeded walks of it."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge


def run(n_walks=4, seed=0, log=print, n_ops=400, shapes=None, dry=False, calls=False):
    """n_walks walks per shape from seeds seed, seed + 1, ...; returns the number of walks that failed.
    dry: no device (the model against itself); calls: a line per call as well."""
    import session_model as sm
    pkg, orc = ge.load_package(), ge.load_oracle()
    orc.lib()
    B = None
    if not dry:
        B = pkg.binding
        B.lib()
        assert B.device_count() >= 1, "no HIP device (dry=True walks the model alone)"
    bad = 0
    for shape in shapes or list(sm.SHAPES):
        world = sm.World(pkg.checkpoint, orc, shape, gpu=B)
        for k in range(n_walks):
            try:
                st = sm.run(world, seed + k, n_ops=n_ops, log=log if calls else None)
                ops = " ".join(f"{name}:{n}" for name, n in sorted(st["ops"].items()))
                log(f"ok  {shape} seed {seed + k}: {st['calls']} operations {st['wall']:.2f} s, worst err/bar {st['worst']:.3f} "
                    f"({st['worst_at']}), under margin {st['id_under']}/{st['id_total']}, refusals {dict(st['refusals'])}\n    {ops}")
            except sm.WalkFailure as e:
                bad += 1
                log(f"BAD {shape} seed {seed + k}: {e}")
        world.close()
    return bad


if __name__ == "__main__":
    a = sys.argv[1:]
    n_bad = run(int(a[0]) if len(a) > 0 else 4, int(a[1]) if len(a) > 1 else 0, n_ops=int(a[2]) if len(a) > 2 else 400,
                shapes=[a[3]] if len(a) > 3 else None, dry=os.environ.get("FUZZ_SESSION_DRY") == "1")
    sys.exit(1 if n_bad else 0)
