"""rz_destroy gives back what a context held.  Nothing names the context's device buffers one by one any more (a DevBuf frees
itself: DESIGN.md 4.3), so this is the check that none of them outlives its context."""
import numpy as np
import pytest
import torch

from rayzen_amd import scene as S
from rayzen_amd.renderer import Renderer, frame_params

pytestmark = pytest.mark.gpu

MIB = 1 << 20
SIZE = 1024         # the accumulation is 16 MiB, the denoiser's guide 32 MiB, its two ping-pong buffers 16 MiB each
CYCLES = 4


def _cycle(sc):
    r = Renderer(0)
    r.upload_scene(sc)
    r.set_frame(frame_params(sc.camera, SIZE, SIZE, len(sc.lights), 1, 1))
    r.render()
    r.present_denoised()
    n = sc.arrays[S.BIND_TRIANGLES].shape[0]
    skin = np.zeros(n, S.SKIN_TRIANGLE)
    skin["weights"][:, :, 0] = 1.0
    rig = r.skin_create(0, n, skin, 1)          # (rest pose: binding 0 as it stands; the rig is left for rz_destroy to free)
    r.skin_pose(rig, bones=np.stack([S.identity()]))
    r.close()
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def test_destroy_returns_the_device_memory_of_a_context():
    """Four create .. destroy cycles of a 1024 x 1024 frame, denoised and presented, with a skin rig posed once.  Cycle 1 absorbs
    what the runtime allocates once; a large buffer leaked per cycle would cost three times its size between the free memory
    after cycle 1 and after cycle 4 -- 48 MiB or more.  The bound is one accumulation buffer, 16 MiB."""
    sc = S.cornell_scene()
    free = [_cycle(sc) for _ in range(CYCLES)]
    lost = free[0] - free[-1]
    print(f"free device memory after each cycle (MiB): {[round(f / MIB, 2) for f in free]}; cycle 1 -> cycle {CYCLES}: {lost / MIB:.2f} MiB lost")
    assert lost < 16 * MIB, f"{lost / MIB:.1f} MiB of device memory did not come back over {CYCLES - 1} create/destroy cycles"
