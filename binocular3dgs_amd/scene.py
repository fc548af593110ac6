"""The part of the reference's `scene/__init__.py` the training loop touches per iteration (train.py:59,127):

    scene.getTrainCameras() / getTestCameras()          scene/__init__.py:90-94
    scene.getShiftedCamera(camera, trans_dist=0.1)      scene/__init__.py:96-115   (the binocular partner)
    scene.cameras_extent                                 scene/__init__.py:64       (densify_and_prune's `extent`)

`Scene(...)` is built from camera.Camera objects the caller already has.  `Scene.from_dataset(source_path, model, ...)` is
the reference's constructor (scene/__init__.py:26-84): dataset_readers reads the COLMAP / Blender folder on the host,
ground_truth.prepare_ground_truth resizes and prepares every image on the device (8 views per call), `input.ply` and
`cameras.json` are written to the model path, the model is created from the initial points or loaded from a saved iteration.
The dense-matcher point cloud itself is not produced here.

`getShiftedCamera` is the closed form SURVEY 8a-9 asks for: in row-vector form only `world_view_transform[3, 0]` moves,
the full projection's last row and the camera centre follow (camera.Camera.shifted, golden G4 against the reference's
construction).  The reference inverts the extrinsic on the device, copies the offset to the host (`.cpu()`: a sync per
iteration) and rebuilds a Camera through two host-side 4x4 inversions, three pageable uploads, a bmm and a device
inverse -- ~0.4 ms of device-idle host work per iteration at the reference's own iteration shape; here: host arithmetic on
cached matrices and ONE asynchronous upload from a pinned ring, no synchronisation.  The returned camera remembers that its
view-space depths equal its parent's (`same_depth_as`), which lets the pair share one depth sort (checked on the device).
"""
from __future__ import annotations

from typing import Sequence


class Scene:
    def __init__(self, train_cameras: Sequence, gaussians=None, test_cameras: Sequence = (), cameras_extent: float = 1.0,
                 model_path: str = ""):
        self.gaussians = gaussians
        self.model_path = model_path
        self.cameras_extent = cameras_extent
        self.train_cameras = {1.0: list(train_cameras)}
        self.test_cameras = {1.0: list(test_cameras)}

    @classmethod
    def from_dataset(cls, source_path: str, model, *, images="images", eval=True, n_views=3, dataset_name="LLFF", suffix=None,
                     resolution=-1, white_background=False, init_points="matcher", model_path=None, shuffle=True,
                     load_iteration=None, device="cuda", depth_priors=None, normal_priors=None,
                     normal_prior_frame="opencv"):
        """scene/__init__.py:26-84.  `model`: a GaussianModel (filled from the initial points, or from
        <model_path>/point_cloud/iteration_<load_iteration>, -1 = the latest) or None (cameras only)."""
        import json
        import os
        import random
        from . import dataset_readers as dr
        info = dr.read_scene(source_path, images=images, eval=eval, n_views=n_views, dataset_name=dataset_name, suffix=suffix,
                             init_points=init_points)
        loaded = None
        if load_iteration:
            from .spiral import max_iteration
            loaded = max_iteration(model_path) if load_iteration == -1 else load_iteration
        train, test = list(info.train_cameras), list(info.test_cameras)
        if model_path and not loaded:
            os.makedirs(model_path, exist_ok=True)
            with open(info.ply_path, "rb") as src, open(os.path.join(model_path, "input.ply"), "wb") as dst:
                dst.write(src.read())
            with open(os.path.join(model_path, "cameras.json"), "w") as fp:
                json.dump([dr.camera_json(i, c) for i, c in enumerate(test + train)], fp)
        if shuffle:
            random.shuffle(train)
            random.shuffle(test)
        thr = None
        if dataset_name == "DTU":
            from .ground_truth import dtu_threshold_for
            thr = dtu_threshold_for(source_path)
        scene = cls(_load_cameras(train, resolution, white_background, thr, device), model,
                    _load_cameras(test, resolution, white_background, thr, device), info.radius, model_path or "")
        scene.loaded_iter, scene.scene_info = loaded, info
        if depth_priors:
            # <depth_priors>/<image_name>.npy of every TRAINING view -> Camera.depth_prior / depth_prior_mask at its size
            from .depth_prior import attach_priors
            attach_priors(depth_priors, scene.getTrainCameras(), device=device)
        if normal_priors:
            # <normal_priors>/<image_name>.npy | .png of every TRAINING view -> Camera.normal_prior / normal_prior_mask
            from .normal_prior import attach_normal_priors
            attach_normal_priors(normal_priors, scene.getTrainCameras(), frame=normal_prior_frame, device=device)
        if model is not None:
            if loaded:
                model.load_ply(os.path.join(model_path, "point_cloud", "iteration_" + str(loaded), "point_cloud.ply"))
            else:
                model.create_from_pcd(dr.PointCloud(info.points, info.colors), info.radius)
        return scene

    def getTrainCameras(self, scale=1.0):
        return self.train_cameras[scale]

    def getTestCameras(self, scale=1.0):
        return self.test_cameras[scale]

    def getShiftedCamera(self, camera, trans_dist=0.1):
        return getShiftedCamera(camera, trans_dist)

    def save(self, iteration):
        """scene/__init__.py:86-88"""
        import os
        self.gaussians.save_ply(os.path.join(self.model_path, "point_cloud", f"iteration_{iteration}", "point_cloud.ply"))


def _load_cameras(infos, resolution, white_background, dtu_threshold, device):
    """utils/camera_utils.py:47-53 cameraList_from_camInfos: one Camera per CameraInfo, uid = position in the list.  The images
    are decoded one batch ahead of the device at most and grouped by output size."""
    from . import dataset_readers as dr
    from .camera import Camera
    from .ground_truth import output_size, prepare_ground_truth
    sizes = [output_size(*dr.image_size(c.image_path), resolution) for c in infos]
    gts = [None] * len(infos)
    for size in dict.fromkeys(sizes):
        idx = [i for i, s in enumerate(sizes) if s == size]
        prepared = prepare_ground_truth((dr.read_image(infos[i].image_path) for i in idx), size,
                                        white_background=white_background, dtu_threshold=dtu_threshold, device=device)
        for i, g in zip(idx, prepared):
            gts[i] = g
    return [Camera(c.R, c.T, c.FovX, c.FovY, sizes[i][0], sizes[i][1], image=gts[i][0], gt_alpha_mask=gts[i][1], uid=i,
                   device=device, prepared=True, image_name=c.image_name, colmap_id=c.uid, bg_mask=gts[i][2])
            for i, c in enumerate(infos)]


def getShiftedCamera(camera, trans_dist=0.1):
    """scene/__init__.py:96-115 for a camera.Camera: centre moved by `trans_dist` along the camera's own +x axis, image of
    ones, no alpha mask, same R / T / FoV / uid."""
    return camera.shifted(float(trans_dist))
