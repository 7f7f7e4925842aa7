"""The evaluation model with inserted lamps: tester.test_model.MaterialModel plus one conf key the reference does not have.

    test.lights = none | <json of inserted emitters, the file form of train.irt_lights (irtlight.load)>
    test.light_samples = 64

With lights, render() adds their diffuse and specular response to every rendered view, sum_k colour_k (albedo / pi F[k] + R[k]) (Scene.irt_lights,
Scene.spec_lights, irtlight.add_view), at test.light_samples samples per pixel, light and technique, with the pixels' own specular shift and the model's
floor of denominators.  With the default `none` the class IS its base: every file Editing, View, Relighting and Error write is unchanged byte for byte.
This is the class the plugin registry hands the tester runners for models.test_nvdiffrast.MaterialModel."""
import torch

from .. import irtlight
from . import test_model as TM


def load_test_lights(spec, device):
    """test.lights: 'none' -> None; a json path (irtlight.load) -> (records [K,16], colours [K,3]) on the device"""
    if spec.lower() == "none":
        return None
    records, colours = irtlight.load(spec)
    return torch.from_numpy(records).to(device), torch.from_numpy(colours).to(device)


class MaterialModel(TM.MaterialModel):
    def __init__(self, conf, *args, **kwargs):
        super().__init__(conf, *args, **kwargs)
        self.test_lights = load_test_lights(str(conf.get("test.lights", "none")), self.device)
        self.light_samples = int(conf.get("test.light_samples", 64))

    def render(self, normal, albedo, roughness, points, cam_position, irr):
        lights = getattr(self, "test_lights", None)
        if lights is None:
            return super().render(normal, albedo, roughness, points, cam_position, irr)
        # The base draws the pixels' specular shift from the CPU generator and keeps it to itself.  The same numbers are drawn again from a private
        # generator started at the state the base found: the CPU generator itself sees the base's draws and no further one.
        replay = torch.Generator()
        replay.set_state(torch.get_rng_state())
        res = super().render(normal, albedo, roughness, points, cam_position, irr)
        shape = tuple(normal.shape[:-1])
        P = normal.numel() // 3
        if self.relighting:
            torch.rand(P, 1, 2, generator=replay)                                        # the diffuse term's draw comes first (test_model.render)
        shift_s = torch.rand(P, 1, 2, generator=replay).reshape(P, 2).to(self.device)
        records, colours = lights
        n_l = int(getattr(self, "light_samples", 64))
        pts, nrm, alb = points.reshape(P, 3), normal.reshape(P, 3), albedo.reshape(P, 3)
        F = self.scene.irt_lights(pts, nrm, shift_s, records, n_l)
        R = self.scene.spec_lights(pts, nrm, roughness.reshape(P), shift_s, cam_position, records, n_l, clamp_eps=TM.TINY_NUMBER)
        res["rgb"] = irtlight.add_view(res["rgb"].reshape(P, 3), alb, F, R, colours).reshape(shape + (3,))
        return res
