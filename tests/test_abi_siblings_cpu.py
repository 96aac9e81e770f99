"""CPU: each depth-gated (or near-clipped) entry of the C ABI checks what its sibling checks, in the sibling's order, with the
gate's own checks at a pinned place among them.  Every pointer is a dummy that is never dereferenced (the seed grid's lo and
step are read, so they are real); no row passes validation with work to do, so nothing is launched."""
import ctypes

A = ctypes.c_void_p(64)
NAN, INF = float("nan"), float("inf")


def _d3(*v):
    return (ctypes.c_double * 3)(*v)


_GRID = dict(nx=4, ny=5, nz=6, lo=_d3(0.0, 0.0, 0.0), step=_d3(0.1, 0.1, 0.1))
_BAD_STEP = _d3(0.1, 0.0, 0.1)
_GATE = dict(depth=A, slack=0.5)
_SLACK = "(slack={}; the slack is finite and >= 0)"
_PLANE = "(near={}; the plane is finite and > 0)"


def each(value, names):
    return [{n: value} for n in names.split()]


def _slack_rows(first_pointer_message):
    return [(dict(slack=-0.5), _SLACK.format("-0.5")), (dict(slack=NAN), _SLACK.format("nan")),
            (dict(slack=INF), _SLACK.format("inf")), (dict(depth=None), first_pointer_message)]


def _near_rows():
    return [(dict(near=0.0), _PLANE.format("0")), (dict(near=-0.5), _PLANE.format("-0.5")),
            (dict(near=NAN), _PLANE.format("nan")), (dict(near=INF), _PLANE.format("inf"))]


# One record per pair: the sibling's name and arguments, the gated entry's suffix and arguments, the values of a valid call,
# the gate's valid values, the rows that both take (a dict of broken arguments each), and the gated entry's own rows with
# the text after "<entry>: invalid argument " written out (None: the call is a no-op that returns 0).
_PAIRS = [
    dict(fn="cgs_edge_visibility", suffix="_depth",
         names="n_curves curves n_lines lines n_frames K w2c height width maps invert counts stream",
         gated="n_curves curves n_lines lines n_frames K w2c height width maps invert depth slack counts stream",
         base=dict(n_curves=3, n_lines=2, n_frames=2, height=8, width=16, invert=0), gate=_GATE,
         rows=[dict(n_curves=-1), dict(n_lines=-1), dict(n_frames=-1), dict(n_curves=1 << 30, n_lines=1),
               dict(n_curves=0, n_lines=0), dict(n_curves=0, n_lines=0, height=0), dict(n_curves=0, n_lines=0, counts=None),
               dict(n_curves=-1, n_lines=0), dict(height=0), dict(width=-1), dict(n_frames=0, height=0, counts=None),
               dict(n_curves=-1, height=0), dict(height=0, counts=None), dict(n_curves=0, curves=None, counts=None),
               dict(n_lines=0, lines=None, K=None)] + each(None, "curves lines counts K w2c maps"),
         own=_slack_rows("(NULL pointer)") + [
             (dict(n_curves=-1, slack=-0.5), "(n_curves=-1, n_lines=2, n_frames=2)"),
             (dict(n_curves=0, n_lines=0, slack=-0.5), _SLACK.format("-0.5")),
             (dict(slack=NAN, height=0), _SLACK.format("nan")), (dict(depth=None, height=0), "(height=0, width=16)"),
             (dict(n_frames=0, depth=None, counts=None), "(NULL pointer)"), (dict(n_curves=0, n_lines=0, depth=None), None)]),
    dict(fn="cgs_project_points", suffix="_depth", names="P points V intr w2c height width uv_out stream",
         gated="P points V intr w2c height width depth slack uv_out hidden stream",
         base=dict(P=5, V=2, height=8, width=16), gate=_GATE,
         rows=[dict(P=-1), dict(V=-1), dict(P=1 << 30, V=1 << 20), dict(P=0), dict(V=0), dict(P=0, height=0),
               dict(V=0, points=None), dict(P=-1, V=0), dict(height=0), dict(width=0), dict(height=0, points=None),
               dict(P=-1, height=0)] + each(None, "points intr w2c uv_out"),
         own=_slack_rows("(NULL pointer)") + [
             (dict(P=-1, slack=-0.5), "(P=-1, V=2)"), (dict(slack=-0.5, P=0), _SLACK.format("-0.5")),
             (dict(slack=INF, height=0), _SLACK.format("inf")), (dict(depth=None, height=0), "(height=0, width=16)"),
             (dict(V=0, depth=None), None), (dict(hidden=None, depth=None), "(NULL pointer)")]),
    dict(fn="cgs_render_points", suffix="_depth",
         names="P points colors V intr w2c height width alpha background out kept workspace workspace_bytes stream",
         gated="P points colors V intr w2c height width depth slack alpha background out kept hidden workspace "
               "workspace_bytes stream",
         base=dict(P=5, V=2, height=8, width=16, alpha=0.5, workspace_bytes=1 << 30), gate=_GATE,
         rows=[dict(P=-1), dict(V=-1), dict(height=0), dict(width=0), dict(height=65536, width=65536), dict(alpha=-0.1),
               dict(alpha=1.5), dict(alpha=NAN), dict(V=0), dict(V=0, intr=None), dict(V=0, workspace_bytes=0),
               dict(V=0, alpha=2.0), dict(height=0, alpha=2.0), dict(alpha=2.0, out=None),
               dict(P=0, points=None, colors=None, intr=None), dict(workspace_bytes=0), dict(workspace_bytes=0, out=None)]
         + each(None, "intr w2c background out workspace points colors"),
         own=_slack_rows("(NULL pointer)") + [
             (dict(height=0, slack=-0.5), "(P=5, V=2, height=0, width=16)"), (dict(slack=-0.5, alpha=2.0), _SLACK.format("-0.5")),
             (dict(slack=NAN, V=0), _SLACK.format("nan")), (dict(depth=None, alpha=2.0), "(alpha=2, need 0 <= alpha <= 1)"),
             (dict(depth=None, workspace_bytes=0), "(NULL pointer)"), (dict(V=0, depth=None), None)]),
    dict(fn="cgs_voxel_votes", suffix="_depth",
         names="nx ny nz lo step V intr w2c height width bits accumulate seen hit stream",
         gated="nx ny nz lo step V intr w2c height width bits depth slack accumulate seen hit hidden stream",
         base=dict(_GRID, V=2, height=8, width=16, accumulate=1), gate=_GATE,
         rows=[dict(V=-1), dict(V=65536), dict(height=0), dict(width=0), dict(nx=0), dict(ny=-1), dict(nz=0),
               dict(nx=65536, ny=65536), dict(nx=2048, ny=2048, nz=2048), dict(lo=_d3(NAN, 0.0, 0.0)), dict(step=_BAD_STEP),
               dict(step=_d3(0.1, 0.1, INF)), dict(lo=None, step=_BAD_STEP), dict(step=_BAD_STEP, seen=None),
               dict(nx=0, lo=None), dict(V=-1, nx=0), dict(V=0), dict(V=0, intr=None, w2c=None, bits=None),
               dict(V=0, seen=None), dict(V=0, step=_BAD_STEP)] + each(None, "lo step seen hit intr w2c bits"),
         own=_slack_rows("(NULL pointer)") + [
             (dict(nx=0, slack=-0.5), "(dims=0x5x6)"), (dict(step=_BAD_STEP, slack=-0.5), "(axis 1: lo=0, step=0)"),
             (dict(slack=-0.5, seen=None), _SLACK.format("-0.5")), (dict(slack=INF, V=0), _SLACK.format("inf")),
             (dict(step=_BAD_STEP, depth=None), "(NULL pointer)"), (dict(V=0, depth=None), None)]),
    dict(fn="cgs_ray_claims", suffix="_depth",
         names="nx ny nz lo step M index support V intr w2c height width bits clear best stream",
         gated="nx ny nz lo step M index support V intr w2c height width bits depth slack clear best stream",
         base=dict(_GRID, M=3, V=2, height=8, width=16, clear=1), gate=_GATE,
         rows=[dict(M=-1), dict(V=-1), dict(height=0), dict(width=16385), dict(nx=0), dict(lo=_d3(0.0, INF, 0.0)),
               dict(step=_BAD_STEP), dict(M=0, lo=None), dict(V=0, step=None), dict(M=-1, V=-1), dict(lo=None, nx=0),
               dict(lo=None, step=_BAD_STEP), dict(step=_BAD_STEP, best=None), dict(M=0, V=0, lo=None),
               dict(M=0, index=None, best=None)] + each(None, "lo step best index support intr w2c bits"),
         own=_slack_rows("(NULL pointer)") + [
             (dict(nx=0, slack=-0.5), "(dims=0x5x6)"), (dict(step=_BAD_STEP, slack=-0.5), "(axis 1: lo=0, step=0)"),
             (dict(slack=-0.5, lo=None), _SLACK.format("-0.5")), (dict(slack=NAN, M=0, V=0), _SLACK.format("nan")),
             (dict(M=0, depth=None, best=None), "(NULL pointer)")]),
    dict(fn="cgs_ray_wins", suffix="_depth",
         names="nx ny nz lo step M index support V intr w2c height width bits best window margin accumulate wins stream",
         gated="nx ny nz lo step M index support V intr w2c height width bits best depth slack window margin accumulate wins "
               "stream",
         base=dict(_GRID, M=3, V=2, height=8, width=16, window=2, margin=1, accumulate=0), gate=_GATE,
         rows=[dict(M=-1), dict(V=-1), dict(width=0), dict(nz=0), dict(step=_BAD_STEP), dict(lo=None), dict(step=None),
               dict(lo=None, window=-1), dict(window=-1), dict(window=5), dict(margin=-1), dict(margin=65536),
               dict(window=-1, wins=None), dict(M=0), dict(V=0), dict(M=0, index=None, wins=None), dict(M=0, window=-1),
               dict(V=0, margin=-1), dict(M=0, lo=None), dict(M=-1, nz=0)]
         + each(None, "index support intr w2c bits best wins"),
         own=_slack_rows("(NULL pointer)") + [
             (dict(slack=-0.5, window=-1), _SLACK.format("-0.5")), (dict(lo=None, slack=-0.5), "(NULL pointer)"),
             (dict(step=_BAD_STEP, slack=-0.5), "(axis 1: lo=0, step=0)"), (dict(slack=INF, wins=None), _SLACK.format("inf")),
             (dict(M=0, slack=NAN), _SLACK.format("nan")), (dict(M=0, depth=None), None),
             (dict(depth=None, window=-1),
              "(window=-1, margin=1; the window lies in [0, 4], the margin in [0, 65535])")]),
    dict(fn="cgs_edge_support", suffix="_depth",
         names="E P points offsets V intr w2c height width d2 T tol2 counts stream",
         gated="E P points offsets V intr w2c height width d2 T tol2 depth slack counts hidden stream",
         base=dict(E=3, P=10, V=2, height=8, width=16, T=2), gate=_GATE,
         rows=[dict(E=-1), dict(P=-1), dict(V=-1), dict(T=0), dict(T=5), dict(E=0), dict(V=0), dict(E=0, height=0),
               dict(V=0, offsets=None), dict(E=0, T=0), dict(height=0), dict(width=16385), dict(height=0, offsets=None),
               dict(T=0, height=0), dict(P=0, points=None, counts=None)]
         + each(None, "offsets intr w2c d2 tol2 counts points"),
         own=_slack_rows("(NULL pointer)") + [
             (dict(T=0, slack=-0.5), "(E=3, P=10, V=2, T=0; T lies in [1, 4])"), (dict(slack=-0.5, E=0), _SLACK.format("-0.5")),
             (dict(slack=NAN, height=0), _SLACK.format("nan")), (dict(E=0, depth=None), None),
             (dict(height=0, depth=None), "(height=0, width=16; sizes lie in [1, 16384])")]),
    dict(fn="cgs_sample_support", suffix="_depth", names="P points V intr w2c height width d2 T tol2 tally stream",
         gated="P points V intr w2c height width d2 T tol2 depth slack tally hidden stream",
         base=dict(P=10, V=2, height=8, width=16, T=2), gate=_GATE,
         rows=[dict(P=-1), dict(V=-1), dict(T=0), dict(T=5), dict(height=0), dict(width=0), dict(T=0, height=0),
               dict(height=0, intr=None), dict(P=0), dict(V=0), dict(P=0, points=None, tally=None), dict(P=0, intr=None),
               dict(V=0, d2=None), dict(P=0, height=0)] + each(None, "intr w2c d2 tol2 points tally"),
         own=_slack_rows("(NULL pointer; P=10, V=2)") + [
             (dict(height=0, slack=-0.5), "(height=0, width=16; sizes lie in [1, 16384])"),
             (dict(slack=-0.5, intr=None), _SLACK.format("-0.5")), (dict(slack=INF, P=0), _SLACK.format("inf")),
             (dict(P=0, depth=None), "(NULL pointer; P=0, V=2)"), (dict(P=0, hidden=None), None)]),
    dict(fn="cgs_sample_support_oriented", suffix="_depth",
         names="P points partner V intr w2c height width near spread tally stream",
         gated="P points partner V intr w2c height width near spread depth slack tally hidden stream",
         base=dict(P=10, V=2, height=8, width=16, spread=1), gate=_GATE,
         rows=[dict(P=-1), dict(V=-1), dict(spread=-1), dict(spread=5), dict(height=0), dict(width=0), dict(spread=-1, height=0),
               dict(height=0, intr=None), dict(P=0), dict(V=0), dict(P=0, points=None, partner=None, tally=None),
               dict(P=0, near=None), dict(V=0, intr=None), dict(V=0, width=0)]
         + each(None, "intr w2c near points partner tally"),
         own=_slack_rows("(NULL pointer; P=10, V=2)") + [
             (dict(width=0, slack=-0.5), "(height=8, width=0; sizes lie in [1, 16384])"),
             (dict(slack=-0.5, near=None), _SLACK.format("-0.5")), (dict(slack=NAN, V=0), _SLACK.format("nan")),
             (dict(V=0, depth=None), "(NULL pointer; P=10, V=0)"), (dict(V=0, hidden=None), None)]),
    dict(fn="cgs_sample_snap_terms", suffix="_depth",
         names="P points V intr w2c height width d2 cap2 dist_lut terms views stream",
         gated="P points V intr w2c height width d2 cap2 dist_lut depth slack terms views hidden stream",
         base=dict(P=10, V=2, height=8, width=16, cap2=4), gate=_GATE,
         rows=[dict(P=-1), dict(V=-1), dict(cap2=0), dict(cap2=65), dict(height=0), dict(width=0), dict(cap2=0, height=0),
               dict(height=0, d2=None), dict(P=0), dict(V=0), dict(P=0, points=None, terms=None, views=None),
               dict(P=0, dist_lut=None), dict(V=0, w2c=None), dict(P=0, height=16385)]
         + each(None, "intr w2c d2 dist_lut points terms views"),
         own=_slack_rows("(NULL pointer; P=10, V=2)") + [
             (dict(height=0, slack=-0.5), "(height=0, width=16; sizes lie in [1, 16384])"),
             (dict(slack=-0.5, dist_lut=None), _SLACK.format("-0.5")), (dict(slack=INF, P=0), _SLACK.format("inf")),
             (dict(P=0, depth=None), "(NULL pointer; P=0, V=2)"), (dict(P=0, hidden=None), None)]),
    dict(fn="cgs_mesh_depth", suffix="_clipped", names="F tris V intr w2c height width depth stream",
         gated="F tris V intr w2c height width near depth stream",
         base=dict(F=3, V=2, height=8, width=16), gate=dict(near=0.01),
         rows=[dict(F=-1), dict(V=-1), dict(height=0), dict(width=0), dict(F=-1, height=0), dict(height=0, depth=None),
               dict(V=0), dict(V=0, tris=None), dict(F=0, tris=None, depth=None), dict(V=0, F=0, tris=None), dict(V=0, width=0)]
         + each(None, "intr w2c depth tris"),
         own=_near_rows() + [(dict(height=0, near=0.0), "(height=0, width=16; sizes lie in [1, 16384])"),
                             (dict(near=0.0, intr=None), _PLANE.format("0")), (dict(near=NAN, V=0), _PLANE.format("nan")),
                             (dict(near=INF, F=0, tris=None), _PLANE.format("inf"))]),
    dict(fn="cgs_mesh_contours", suffix="_clipped", names="E edges V intr w2c height width depth slack mask_out stream",
         gated="E edges V intr w2c height width depth slack near mask_out stream",
         base=dict(E=3, V=2, height=8, width=16, slack=0.001), gate=dict(near=0.01),
         rows=[dict(E=-1), dict(V=-1), dict(height=0), dict(width=0), dict(slack=-0.5), dict(slack=NAN), dict(slack=INF),
               dict(depth=None, slack=-0.5, intr=None), dict(height=0, slack=-0.5), dict(slack=-0.5, intr=None),
               dict(slack=-0.5, V=0), dict(V=0), dict(V=0, depth=None, slack=NAN), dict(V=0, mask_out=None),
               dict(E=0, edges=None, intr=None), dict(E=-1, height=0)] + each(None, "intr w2c mask_out edges"),
         own=_near_rows() + [
             (dict(slack=-0.5, near=0.0), "(slack=-0.5; with a depth plane the slack is finite and >= 0)"),
             (dict(height=0, near=0.0), "(height=0, width=16; sizes lie in [1, 16384])"),
             (dict(near=0.0, intr=None), _PLANE.format("0")), (dict(depth=None, slack=NAN, near=INF), _PLANE.format("inf")),
             (dict(near=NAN, V=0), _PLANE.format("nan")), (dict(depth=None, slack=NAN, V=0), None)]),
]


def _call(lib, fn, names, values):
    from curve_gaussian_amd import _lib
    names = names.split()
    assert len(names) == len(_lib.SIGNATURES[fn][1]) and set(values) <= set(names), (fn, sorted(set(values) - set(names)))
    values = dict({n: A for n in names}, stream=None, **{k: v for k, v in values.items() if k != "stream"})
    rc = getattr(lib, fn)(*[values[n] for n in names])
    return rc, lib.cgs_last_error().decode()


def test_every_pair_is_listed_once():
    assert len(_PAIRS) == 12 and len({p["fn"] for p in _PAIRS}) == 12
    for p in _PAIRS:
        assert set(p["gated"].split()) - set(p["names"].split()) <= set(p["gate"]) | {"hidden"}, p["fn"]
        assert len(p["rows"]) >= 12 and len(p["own"]) >= 8, p["fn"]


def test_siblings_reject_the_same_rows_with_the_same_text():
    from curve_gaussian_amd import _lib
    lib = _lib.load()
    for p in _PAIRS:
        fn, gated = p["fn"], p["fn"] + p["suffix"]
        seen = set()
        for changes in p["rows"]:
            assert changes, fn
            rc, text = _call(lib, fn, p["names"], dict(p["base"], **changes))
            assert rc in (0, -1), (fn, changes, rc, text)   # rejected, or a no-op: never launched
            rc_g, text_g = _call(lib, gated, p["gated"], dict(p["base"], **dict(p["gate"], **changes)))
            assert rc_g == rc, (gated, changes, rc_g, text_g)
            if rc < 0:
                assert text.startswith(fn + ": invalid argument ("), (fn, changes, text)
                assert text_g == gated + text[len(fn):], (gated, changes)
                seen.add(text)
        assert len(seen) >= 3, fn   # the rows reach several checks of the body


def test_gated_entries_place_their_own_checks():
    from curve_gaussian_amd import _lib
    lib = _lib.load()
    for p in _PAIRS:
        gated = p["fn"] + p["suffix"]
        for changes, message in p["own"]:
            rc, text = _call(lib, gated, p["gated"], dict(p["base"], **dict(p["gate"], **changes)))
            assert rc == (0 if message is None else -1), (gated, changes, rc, text)
            if message is not None:
                assert text == f"{gated}: invalid argument {message}", (gated, changes)
