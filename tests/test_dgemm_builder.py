"""pika_dgemm_t as its callers fill it: `dgemm_args` (pika_amd/decoder/fused_step.py) against the structs that
`FusedSearch._gemm` and the `dgemm` closure of `LASDecoder._prepare_fused` filled field by field before the builder
existed, written out here by hand and compared byte for byte.  No GPU, no library: pointers are made-up addresses."""
import ctypes
import types

import pytest

from pika_amd.decoder import fused_step as fs
from pika_amd.decoder.fused_step import DGemm, dgemm_args

RELU, GATE, FEW = fs.DG_RELU, fs.DG_GATE, fs.DG_FEW_ROWS


class Ptr(object):
    """Stands for a tensor: an address and nothing else."""
    def __init__(self, addr):
        self.addr = addr

    def data_ptr(self):
        return self.addr


def weight(addr, N, K, terms):
    return types.SimpleNamespace(buf=Ptr(addr), N=N, K=K, terms=terms)


def frozen(**values):
    g = DGemm()
    for k, v in values.items():
        assert k in dict(DGemm._fields_), k
        setattr(g, k, v)
    return g


# ---- FusedSearch._gemm ------------------------------------------------------------------------------------------
R, D, HID, H, T, BEAM, DUMP = 1024, 512, 2048, 640, 77, 16, 300001
NODE, E_ALL, T_IDX = 0x1000, 0x2000, 0x3000
SELF = types.SimpleNamespace(node=Ptr(NODE), dump_node=DUMP, e_all=Ptr(E_ALL), t_idx=Ptr(T_IDX), T=T, K=BEAM)
COMMON = dict(node=NODE, skip_node=DUMP, e_all=E_ALL, t_idx=T_IDX, T=T, beam=BEAM)
LN = types.SimpleNamespace(weight=Ptr(0x7000), bias=Ptr(0x7100), eps=1e-6)
A, C, RES, C2, COUNT, CROW, RL = Ptr(0x10000), Ptr(0x20000), Ptr(0x30000), Ptr(0x40000), Ptr(0x50), Ptr(0x60), Ptr(0x70)
W, BIAS = weight(0x100000, 1536, D, 4), Ptr(0x8000)

GEMM_CASES = {
    "conv": (dict(args=(A, 5 * D, weight(0x100000, D, 5 * D, 4), BIAS, C, D, R), kw=dict(relu=True, m_dev=COUNT)),
             dict(A=0x10000, lda=5 * D, W=0x100000, bias=0x8000, C=0x20000, ldc=D, M=R, N=D, K=5 * D, terms=4,
                  flags=RELU | FEW, m_dev=0x50, **COMMON)),
    "qkv+ln": (dict(args=(A, D, W, BIAS, C, 3 * D, R), kw=dict(m_dev=COUNT, ln=LN)),
               dict(A=0x10000, lda=D, W=0x100000, bias=0x8000, C=0x20000, ldc=3 * D, M=R, N=1536, K=D, terms=4, flags=FEW,
                    m_dev=0x50, ln_gamma=0x7000, ln_beta=0x7100, ln_eps=1e-6, **COMMON)),
    "fin+res": (dict(args=(A, D, weight(0x100000, D, D, 3), BIAS, C, D, R), kw=dict(res=RES, ldr=D, m_dev=COUNT)),
                dict(A=0x10000, lda=D, W=0x100000, bias=0x8000, C=0x20000, ldc=D, M=R, N=D, K=D, terms=3, flags=FEW,
                     res=0x30000, ldr=D, m_dev=0x50, **COMMON)),
    "w2+C2": (dict(args=(A, HID, weight(0x100000, D, HID, 4), BIAS, C, 5 * D, R),
                   kw=dict(res=RES, ldr=D, C2=C2, ldc2=D, m_dev=COUNT)),
              dict(A=0x10000, lda=HID, W=0x100000, bias=0x8000, C=0x20000, ldc=5 * D, M=R, N=D, K=HID, terms=4, flags=FEW,
                   res=0x30000, ldr=D, C2=0x40000, ldc2=D, m_dev=0x50, **COMMON)),
    "w2+crow": (dict(args=(A, HID, weight(0x100000, D, HID, 4), BIAS, C, D, R),
                     kw=dict(res=RES, ldr=D, m_dev=COUNT, crow=CROW)),
                dict(A=0x10000, lda=HID, W=0x100000, bias=0x8000, C=0x20000, ldc=D, M=R, N=D, K=HID, terms=4, flags=FEW,
                     res=0x30000, ldr=D, m_dev=0x50, crow=0x60, **COMMON)),
    "gated joint": (dict(args=(A, D, weight(0x100000, 2 * H, D, 2), None, C, H, R),
                         kw=dict(gate=True, m_dev=COUNT, rowlist=RL, C2=C2, ldc2=2 * H, ln=LN)),
                    dict(A=0x10000, lda=D, W=0x100000, C=0x20000, ldc=H, M=R, N=2 * H, K=D, terms=2, flags=GATE | FEW,
                         C2=0x40000, ldc2=2 * H, m_dev=0x50, rowlist=0x70, ln_gamma=0x7000, ln_beta=0x7100, ln_eps=1e-6,
                         **COMMON)),
    "final_state": (dict(args=(A, D, weight(0x100000, H, D, 4), BIAS, C, H, R), kw=dict(ln=LN)),
                    dict(A=0x10000, lda=D, W=0x100000, bias=0x8000, C=0x20000, ldc=H, M=R, N=H, K=D, terms=4, flags=0,
                         ln_gamma=0x7000, ln_beta=0x7100, ln_eps=1e-6, **COMMON)),
}


@pytest.mark.parametrize("name", sorted(GEMM_CASES))
def test_fused_search_gemm(name, monkeypatch):
    call, want = GEMM_CASES[name]
    seen = []

    class Lib(object):
        @staticmethod
        def pika_dgemm(ref, stream):
            seen.append(bytes(ref._obj))
            return 0
    monkeypatch.setattr(fs, "_lib", types.SimpleNamespace(lib=lambda: Lib, check=lambda rc, what: None))
    monkeypatch.setattr(fs, "_stream", lambda: 0)
    fs.FusedSearch._gemm(SELF, *call["args"], **call["kw"])
    assert seen == [bytes(frozen(**want))]


# ---- the dgemm closure of LASDecoder._prepare_fused: flags = 0 (the launch is sized by n_max), skip_node = -1, node = iden
# only with C2, the step's active rows as a gather list ---------------------------------------------------------------
N_MAX, LH, LE = 470, 1024, 512
N_DEV, QLIST, QOFF, IDEN = Ptr(0x90), Ptr(0xa0), Ptr(0xb0), Ptr(0xc0)


def las_dgemm(A_, lda, W_, bias, C_, ldc, crow_=None, C2_=None, ldc2=0):
    """The closure's call of the builder, as las.py writes it."""
    return dgemm_args(A_, lda, W_, bias, C_, ldc, N_MAX, crow=crow_, C2=C2_, ldc2=ldc2 if C2_ is not None else 0,
                      node=IDEN if C2_ is not None else None, skip_node=-1, m_dev=N_DEV, rowlist=QLIST, rowoff_dev=QOFF)


LAS_LIST = dict(skip_node=-1, M=N_MAX, flags=0, m_dev=0x90, rowlist=0xa0, rowoff_dev=0xb0)
LAS_CASES = {
    "gates": (dict(args=(A, LE + 2 * LH, weight(0x100000, 4 * LH, LE + 2 * LH, 4), BIAS, C, 4 * LH)),
              dict(A=0x10000, lda=LE + 2 * LH, W=0x100000, bias=0x8000, C=0x20000, ldc=4 * LH, N=4 * LH, K=LE + 2 * LH,
                   terms=4, **LAS_LIST)),
    "query": (dict(args=(A, 2 * LH, weight(0x100000, LH, LH, 1), BIAS, C, LH)),
              dict(A=0x10000, lda=2 * LH, W=0x100000, bias=0x8000, C=0x20000, ldc=LH, N=LH, K=LH, terms=1, **LAS_LIST)),
    "output": (dict(args=(A, 2 * LH, weight(0x100000, LH, 2 * LH, 3), BIAS, C, LH),
                    kw=dict(crow_=CROW, C2_=C2, ldc2=LE + 2 * LH)),
               dict(A=0x10000, lda=2 * LH, W=0x100000, bias=0x8000, C=0x20000, ldc=LH, N=LH, K=2 * LH, terms=3,
                    crow=0x60, C2=0x40000, ldc2=LE + 2 * LH, node=0xc0, **LAS_LIST)),
}


@pytest.mark.parametrize("name", sorted(LAS_CASES))
def test_las_closure(name):
    call, want = LAS_CASES[name]
    assert bytes(las_dgemm(*call["args"], **call.get("kw", {}))) == bytes(frozen(**want))


def test_las_source_calls_the_builder_this_way():
    """The keyword expression above is the one in las.py (the closure itself only exists inside a GPU pass)."""
    import inspect
    from pika_amd.model import las
    src = "".join(inspect.getsource(las).split())
    assert ("dgemm_args(A,lda,W,bias,C,ldc,n_max,crow=crow_,C2=C2,ldc2=ldc2ifC2isnotNoneelse0,node=idenifC2isnotNoneelseNone,"
            "skip_node=-1,m_dev=n_dev,rowlist=qlist,rowoff_dev=step[2:3])") in src


def test_unknown_member_is_refused():
    with pytest.raises(AttributeError):
        dgemm_args(A, D, W, BIAS, C, D, R, rowoff=QOFF)


def test_struct_size_matches_header_layout():
    assert ctypes.sizeof(DGemm) == 200
