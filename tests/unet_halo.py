"""Test-side staging of NCHW tensors into the haloed NHWC layout of csrc/unet.hip, shared by the U-Net GPU tests."""
import torch


class Halo:
    """X[(b*(H+2) + y)*(W+2) + x][ld] with one zero pixel all round each image, between zeroed guard rows: W+4 in front (the
    thin weight gradient reads p - (W+2) - 1) and guard_after + W+4 >= W+8 behind (the thin forward reads p0 + 4 + (W+2),
    the 128- and 256-row tile kernels read to the end of their last tile).  device="cpu": the same layout for the tests that
    restate the kernels' row-shifted products on the host."""

    def __init__(self, B, H, W, ld, dtype, guard_after=4096, device="cuda"):
        assert guard_after >= 4
        self.B, self.H, self.W, self.ld = B, H, W, ld
        self.P = B * (H + 2) * (W + 2)
        self.gb = gb = W + 4
        self.store = torch.zeros((gb + self.P + guard_after + W + 4) * ld, dtype=dtype, device=device)
        self.t = self.store[gb * ld:]

    def view(self):
        return self.t[: self.P * self.ld].view(self.B, self.H + 2, self.W + 2, self.ld)

    def rows(self, off=0, n=None):
        """pixel rows [off, off + n) as a matrix [n][ld]; off may reach into the guard rows (n defaults to P)"""
        n = self.P if n is None else n
        return self.store.view(-1, self.ld)[self.gb + off: self.gb + off + n]

    def put(self, x, coff=0):           # x [B,C,H,W] cpu
        self.view()[:, 1:-1, 1:-1, coff:coff + x.shape[1]] = x.permute(0, 2, 3, 1).to(self.t.dtype).to(self.t.device)
        return self

    def get(self, C, coff=0):           # -> [B,C,H,W] cpu fp32 (interior)
        return self.view()[:, 1:-1, 1:-1, coff:coff + C].float().permute(0, 3, 1, 2).cpu().contiguous()

    def halo_is_zero(self):
        v = self.view().float()
        return float(v[:, 0].abs().max() + v[:, -1].abs().max() + v[:, :, 0].abs().max() + v[:, :, -1].abs().max()) == 0.0
