"""Recording stand-ins for the collaborators of a training driver: model, scene, render, optimizer, step.  The reference's
training() (tests/golden/make_train_schedule_golden.py) and this package's train.training() (tests/test_train_driver_cpu.py)
run their real loops on top of them; both write the same call log:

    [iteration, method] or [iteration, "optimizer.step", [groups whose parameter was replaced since the last step]]

for every topology edit, snapshot, report, checkpoint, optimizer step, use_mask switch and the final export.  A replaced
group has no gradient at the next optimizer step (torch.optim.Adam then skips it, train.py:183-236)."""
import torch
from torch import nn

GROUPS = ("f_dc", "f_rest", "opacity", "width", "curve_points", "mask")
# what each edit of scene/topology.py replaces (prune_curves / densification_postfix: every group)
REPLACES = {"densify_and_prune": GROUPS, "prune_curves": GROUPS, "only_prune": GROUPS, "mask_trim_split": ("mask", "curve_points"),
            "curve_split_curvature": GROUPS, "merge_curves": GROUPS, "fix_opacity": ("opacity",),
            "fit_curve_to_line": ("curve_points",)}
ATTR = {"f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "width": "_width",
        "curve_points": "_curve_points", "mask": "_mask"}


class Recorder:
    def __init__(self):
        self.log = []
        self.iteration = 0
        self._use_mask = None

    def add(self, method, *extra):
        self.log.append([self.iteration, method, *extra])

    def use_mask(self, flag):
        if flag != self._use_mask:
            self._use_mask = flag
            self.add("use_mask=%d" % int(flag))


class FakeOptimizer:
    def __init__(self, model):
        self.model = model
        self.param_groups = [{"name": n, "lr": 0.0, "params": []} for n in GROUPS]

    def step(self, *a, **k):
        self.model.rec.add("optimizer.step", sorted(self.model.replaced))
        self.model.replaced.clear()

    def zero_grad(self, set_to_none=False):
        pass


class _NoOpt:
    def step(self, *a, **k):
        pass

    def zero_grad(self, *a, **k):
        pass


class FakeModel:
    """Two curves of 12 splats with real, differentiable tensors (the reference's loss terms read them)."""

    def __init__(self, rec, B=2, m=12):
        self.rec = rec
        self.n_gaussians = m
        g = torch.Generator().manual_seed(0)
        self._curve_points = nn.Parameter(torch.rand(B, 4, 3, generator=g))
        self._width = nn.Parameter(torch.full((B, 1), -4.0))
        self._opacity = nn.Parameter(torch.zeros(B, 1))
        self._mask = nn.Parameter(torch.zeros(B, m, 1))
        self._features_dc = nn.Parameter(torch.zeros(B, m, 1, 1))
        self._features_rest = nn.Parameter(torch.zeros(B, m, 0, 1))
        self.is_bezier = torch.ones(B, dtype=torch.bool)
        self.max_radii2D = torch.zeros(B * m)
        self.replaced = set()
        self.optimizer = FakeOptimizer(self)
        self.exposure_optimizer = _NoOpt()

    def _edit(self, name):
        self.rec.add(name)
        for grp in REPLACES[name]:
            a = ATTR[grp]
            setattr(self, a, nn.Parameter(getattr(self, a).detach().clone()))
            self.replaced.add(grp)

    def densify_and_prune(self, *a, **k):
        self._edit("densify_and_prune")

    def prune_curves(self, mask):
        self._edit("prune_curves")

    def fix_opacity(self):
        self._edit("fix_opacity")

    def only_prune(self, *a):
        self._edit("only_prune")

    def mask_trim_split(self, *a):
        self._edit("mask_trim_split")

    def curve_split_curvature(self, *a):
        self._edit("curve_split_curvature")

    def fit_curve_to_line(self, *a):
        self._edit("fit_curve_to_line")

    def merge_curves(self, *a):
        self._edit("merge_curves")

    def draw_curve(self, *a):
        self.rec.add("draw_curve")

    def draw_ellipsoids(self, *a):
        self.rec.add("draw_ellipsoids")

    def training_setup(self, opt=None):
        pass

    def update_learning_rate(self, iteration):
        self.rec.iteration = iteration

    def oneupSHdegree(self):
        pass

    def add_densification_stats(self, *a):
        pass

    def prepare_scaling_rot(self):
        pass

    def capture(self):
        return {"fake": True}

    def restore(self, params, opt=None):
        pass

    @property
    def n_splats(self):
        return self._curve_points.shape[0] * self.n_gaussians

    @property
    def get_opacity(self):
        return torch.sigmoid(self._opacity).repeat_interleave(self.n_gaussians, 0)

    @property
    def get_curve_opacity(self):
        return torch.sigmoid(self._opacity)

    @property
    def get_curve_width(self):
        return torch.exp(self._width)

    @property
    def get_curve_points(self):
        return self._curve_points

    @property
    def get_xyz(self):
        return self._curve_points[:, :1].expand(-1, self.n_gaussians, -1).reshape(-1, 3)

    @property
    def get_rotation_matrix(self):
        eye = torch.eye(3).expand(self.n_splats, 3, 3)
        return eye + 0.0 * self._curve_points.sum()


class FakeCamera:
    def __init__(self, i):
        self.image_name = f"view{i}"
        self.original_image = torch.full((1, 4, 4), 0.25 * (i % 4))


class FakeScene:
    def __init__(self, rec, gaussians, model_path="fake", n_views=5):
        self.rec = rec
        self.gaussians = gaussians
        self.model_path = model_path
        self.cameras_extent = 1.0
        self._cams = [FakeCamera(i) for i in range(n_views)]

    def getTrainCameras(self, scale=1.0):
        return self._cams

    def getTestCameras(self, scale=1.0):
        return []

    def save(self, iteration):
        self.rec.add("save")


def fake_render(rec):
    def render(viewpoint_cam, gaussians, pipe, bg, use_trained_exp=False, separate_sh=False, use_mask=False, mask_thr=0.01):
        rec.use_mask(bool(use_mask))
        P = gaussians.n_splats
        vsp = torch.zeros(P, 3, requires_grad=True)
        img = gaussians.get_opacity.mean() * torch.ones(1, 4, 4) + vsp.sum()
        radii = torch.ones(P, dtype=torch.int32)
        return {"render": img, "viewspace_points": vsp, "visibility_filter": radii > 0, "radii": radii}
    return render


class FakeStep:
    """What train.training() drives: TrainStep's interface (step / apply_update / drop_update / start_at)."""

    def __init__(self, rec, gaussians, densify_until_iter):
        self.rec, self.g, self.dui = rec, gaussians, densify_until_iter
        self.iteration = 0

    def start_at(self, iteration):
        self.iteration = iteration

    def step(self, update=True):
        self.iteration += 1
        self.g.update_learning_rate(self.iteration)
        self.rec.use_mask(self.iteration >= self.dui)                # TrainStep: use_mask = it >= densify_until_iter
        if update:
            self.g.optimizer.step()
        return torch.tensor(1.0 / self.iteration), {"radii": torch.ones(self.g.n_splats, dtype=torch.int32)}

    def apply_update(self):
        self.g.optimizer.step()      # the groups replaced by this iteration's edits are reported as skipped

    def drop_update(self):
        self.g.replaced.clear()


def normalise(log):
    """The reference writes the snapshot twice per save iteration (train.py:213-229, the same scene.save once more) and draws
    two matplotlib figures (out of scope): one save entry, no draw entries."""
    out = []
    for e in log:
        if e[1].startswith("draw_"):
            continue
        if e[1] == "save" and out and out[-1][:2] == e[:2]:
            continue
        out.append(list(e))
    return out


def compress(log):
    """Optimizer steps that skip nothing as [first, last] runs of iterations; everything else verbatim."""
    runs, rest = [], []
    for e in log:
        if e[1] == "optimizer.step" and not e[2]:
            if runs and runs[-1][1] == e[0] - 1:
                runs[-1][1] = e[0]
            else:
                runs.append([e[0], e[0]])
        else:
            rest.append(list(e))
    return {"plain_steps": runs, "events": rest}
