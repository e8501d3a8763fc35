"""A frozen copy of the edge-weight gradient hand-over as it stood inline in ops.py before the helpers (_dw_to_add, _report_dw,
_take_parked): _handle_grad with its getattr reads, the `second / dw_add / _extra_total` block of the edge-GAT, GATv2 and GINE backwards,
and the three reads of the parked gradient (_GCNNorm, _ChebNorm, _GATEdgeAttr) up to where each hands what it took to its kernel.  Kept
verbatim apart from being cut out of the backwards that held them; the helpers are held to these over every sequence of reporting
layers (tests/test_dw_handover_cpu.py).  Do not edit."""


def handle_grad(nm, g):
    if not getattr(nm, "_park_ok", False):
        return g
    if getattr(nm, "_g_first", None) is None:
        nm._g_first = g
        return g
    if getattr(nm, "_g_extra", None) is None:
        nm._g_extra = g
        return None
    return g


def layer_dw_add(nm, n):
    """The head of the inline block: (second, dw_add) before the layer's kernel forms d w."""
    second = nm._park_ok and nm._g_first is not None and nm._g_extra is None and nm._g_first.numel() == n
    dw_add = nm._g_first.contiguous() if second else None
    return second, dw_add


def layer_report(nm, dw, second, needs_handle_grad):
    """The tail of the inline block: what the layer returns for the handle."""
    g_handle = None
    if needs_handle_grad:
        g_handle = handle_grad(nm, dw)
        if second and g_handle is None:
            nm._extra_total = True
    return g_handle


def gcn_norm_take(nm):
    """_GCNNorm.backward's read: (extra, first)."""
    extra = getattr(nm, "_g_extra", None)
    nm._g_first = nm._g_extra = None
    first = getattr(nm, "_dw_first", None)
    first = first() if first is not None else None
    nm._dw_first = None
    return extra, first


def cheb_norm_take(nm):
    """_ChebNorm.backward's read: extra."""
    extra = getattr(nm, "_g_extra", None)
    nm._g_first = nm._g_extra = None
    return extra


def edge_attr_backward(nm, g):
    """_GATEdgeAttr.backward, whole (it launches nothing): the gradient of the edge weights."""
    extra, total = getattr(nm, "_g_extra", None), getattr(nm, "_extra_total", False)
    nm._g_first = nm._g_extra = None
    nm._extra_total = False
    if extra is None:
        return g
    return extra if total else g + extra
