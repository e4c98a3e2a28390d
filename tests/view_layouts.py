"""The table of operand layouts shared by tests/test_views_cpu.py and tests/test_gpu_views.py: every way a [M, W] fp32 operand can
reach hgn_amd.ops other than as a freshly allocated contiguous tensor, and what ops._rowmajor does with each (its docstring)."""
import torch

LAYOUTS = ('contiguous', 'row_slice', 'col0_of_wider4', 'col_offset1', 'lead_of_wider1', 'transposed', 'expanded', 'every_second_row',
           'float64')
# taken in place whatever the width / only when the width is NOT a multiple of 4 (narrow encoder inputs stay for the masked scalar path)
IN_PLACE = ('contiguous', 'row_slice', 'col0_of_wider4', 'every_second_row')
IN_PLACE_NARROW = IN_PLACE + ('col_offset1', 'lead_of_wider1')
# where the upstream gradient of an operator can sit when autograd hands it over (torch.cat's backward makes the last one by itself)
GRAD_LAYOUTS = ('contiguous', 'col_offset1', 'lead_of_wider1', 'cat_narrow')

# layout -> (rows, columns of the buffer, the view of it) for an [M, W] operand
_BUFFERS = {
    'row_slice': lambda M, W: (M + 5, W, lambda b: b[:M]),
    'col0_of_wider4': lambda M, W: (M, W + 4, lambda b: b[:, :W]),
    'col_offset1': lambda M, W: (M, W + 4, lambda b: b[:, 1:1 + W]),
    'lead_of_wider1': lambda M, W: (M, W + 1, lambda b: b[:, :W]),
    'every_second_row': lambda M, W: (2 * M, W, lambda b: b[::2]),
    'cat_narrow': lambda M, W: (M, W + 3, lambda b: b[:, 3:]),       # what the backward of torch.cat([z[M, 3], y], 1) hands y's producer
}


def copied(layout: str, W: int) -> bool:
    """Whether ops._rowmajor copies an operand of this layout and width."""
    return layout not in (IN_PLACE if W % 4 == 0 else IN_PLACE_NARROW)


class Housed:
    """x's values in `layout`.  `leaf`: the tensor that owns the memory (a wider / taller buffer, NaN wherever the view does not
    reach; requires_grad when asked); `view`: what the operator is handed; `pad`: boolean mask of the buffer's padding, or None.
    (`expanded` repeats x's first row: `values()` is what the operator reads, as a contiguous fp32 tensor.)"""

    def __init__(self, x: torch.Tensor, layout: str, requires_grad: bool = False):
        M, W = x.shape
        self.layout, self.pad = layout, None
        if layout == 'contiguous':
            leaf, f = x.clone(), lambda t: t
        elif layout == 'float64':
            leaf, f = x.double(), lambda t: t
        elif layout == 'transposed':
            leaf, f = x.t().contiguous(), lambda t: t.t()
        elif layout == 'expanded':
            leaf, f = x[:1].clone(), lambda t: t.expand(M, W)
        else:
            rows, cols, f = _BUFFERS[layout](M, W)
            leaf = torch.full((rows, cols), float('nan'), dtype=x.dtype, device=x.device)
            f(leaf).copy_(x)
            self.pad = torch.isnan(leaf)
        self._f = f
        self.leaf = leaf.requires_grad_(requires_grad)
        self.view = f(self.leaf)

    def values(self) -> torch.Tensor:
        return self.view.detach().float().contiguous().clone()

    def of_leaf(self, g):
        """A gradient of `leaf` as the gradient of the [M, W] operand, fp32 (`expanded`: of its one row, i.e. the column sums)."""
        return self._f(g).float() if self.layout != 'expanded' else g

    def grad(self):
        return self.of_leaf(self.leaf.grad)

    def padding_untouched(self) -> bool:
        """The buffer's padding is still NaN, and (after a backward pass) its gradient there is exactly zero."""
        if self.pad is None:
            return True
        ok = bool(torch.isnan(self.leaf.detach()[self.pad]).all()) and bool((~torch.isnan(self.leaf.detach()[~self.pad])).all())
        if self.leaf.grad is not None:
            ok = ok and not bool(self.leaf.grad[self.pad].any()) and bool(torch.isfinite(self.leaf.grad).all())
        return ok


def house(x: torch.Tensor, layout: str):
    """-> (view, buffer or None, padding mask or None)"""
    h = Housed(x, layout)
    return h.view, (h.leaf if h.pad is not None else None), h.pad


def meets_contract(t: torch.Tensor) -> bool:
    """The alignment contract of an operand whose width is a multiple of 4: every row starts on a 16-byte boundary."""
    from hgn_amd import ops
    return t.dtype == torch.float32 and t.stride(1) == 1 and t.data_ptr() % 16 == 0 and ops._ld(t) % 4 == 0


class Rehouse(torch.autograd.Function):
    """Identity whose backward hands the incoming gradient on in another layout (GRAD_LAYOUTS), inside a NaN-padded buffer: put behind
    an operator's output, it decides where that operator's backward finds its upstream gradient.  `log` collects the Housed gradients."""

    @staticmethod
    def forward(ctx, y, layout, log):
        ctx.layout, ctx.log = layout, log
        return y.view_as(y)

    @staticmethod
    def backward(ctx, g):
        h = Housed(g, ctx.layout)
        ctx.log.append((h, g.detach().clone()))
        return h.view, None, None


def rehouse(y, layout, log):
    return y if layout == 'contiguous' else Rehouse.apply(y, layout, log)


def gradients_left_alone(log) -> bool:
    """No backward wrote into the re-housed gradient or its padding."""
    return all(h.padding_untouched() and torch.equal(h.view, g) for h, g in log)
