"""CPU-only: the C-ABI library loads and exports every symbol include/gpode.h declares (no compute)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    txt = open(os.path.join(ROOT, 'include', 'gpode.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(gpode_\w+)\s*\(', txt)))


def test_library_exports_every_declared_symbol():
    from vae_gp_ode_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), 'build first: python -c "import __graft_entry__ as g; g.build()"'
    lib = ctypes.CDLL(_lib.LIB_PATH)
    names = declared_symbols()
    assert len(names) >= 10
    for n in names:
        assert hasattr(lib, n), 'missing export ' + n


def test_binding_table_matches_header():
    from vae_gp_ode_amd import _lib
    assert sorted(_lib.SIGNATURES) == declared_symbols()


def header_prototypes():
    """{name: (return type, [parameter types])} of include/gpode.h: the parameter names stripped, `const` dropped, one space between
    words and none in front of a `*`"""
    txt = open(os.path.join(ROOT, 'include', 'gpode.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    txt = re.sub(r'//[^\n]*|^[ \t]*#[^\n]*|extern\s+"C"\s*\{', '', txt, flags=re.M)

    def ctype(words):
        return re.sub(r'\s*\*', '*', ' '.join(w for w in words.replace('*', ' * ').split() if w != 'const'))
    protos = {}
    for ret, name, params in re.findall(r'([\w\s\*]+?)\b(gpode_\w+)\s*\(([^()]*)\)\s*;', txt):
        assert name not in protos, name
        params = [p.strip() for p in params.split(',')]
        if params in (['void'], ['']):
            params = []
        # `type name`: the name is the last word, and a type never ends in one the header would use for a name
        protos[name] = (ctype(ret), [ctype(re.match(r'(.*?)\w+$', p, flags=re.S).group(1)) for p in params])
    return protos


def signature_mismatches(signatures, protos):
    """every disagreement between a ctypes table and the header's prototypes, by class: any pointer <-> c_void_p, or POINTER(x) with the
    pointee matching; int, float, size_t, (unsigned) long long <-> the ctypes integer / float of that size and signedness; a void return
    <-> None; a `char*` return <-> c_char_p"""
    scalars = {'int': ctypes.c_int, 'float': ctypes.c_float, 'size_t': ctypes.c_size_t, 'long long': ctypes.c_longlong,
               'unsigned long long': ctypes.c_ulonglong}

    def same_scalar(c, t):
        # ctypes makes aliases of the integer types of one size (c_size_t is c_ulong is c_ulonglong on LP64): compare what they are
        want = scalars.get(c)
        return (want is not None and isinstance(t, type) and issubclass(t, ctypes._SimpleCData) and t is not ctypes.c_void_p
                and t is not ctypes.c_char_p and (t._type_ in 'fd') == (want._type_ in 'fd')
                and ctypes.sizeof(t) == ctypes.sizeof(want) and (t(-1).value < 0) == (want(-1).value < 0))

    def agrees(c, t, ret=False):
        if c.endswith('*'):
            if t is ctypes.c_void_p:
                return True
            if ret and c == 'char*':
                return t is ctypes.c_char_p
            return isinstance(t, type) and issubclass(t, ctypes._Pointer) and same_scalar(c[:-1], t._type_)
        if c == 'void':
            return ret and t is None
        return same_scalar(c, t)
    bad = []
    for name in sorted(set(signatures) | set(protos)):
        if name not in signatures or name not in protos:
            bad.append('%s: %s' % (name, 'not in the table' if name in protos else 'not in the header'))
            continue
        (res, args), (cres, cargs) = signatures[name], protos[name]
        if not agrees(cres, res, ret=True):
            bad.append('%s: returns %s, the table has %s' % (name, cres, getattr(res, '__name__', res)))
        if len(args) != len(cargs):
            bad.append('%s: %d parameters, the table has %d' % (name, len(cargs), len(args)))
            continue
        bad += ['%s: parameter %d is %s, the table has %s' % (name, i, c, getattr(t, '__name__', t))
                for i, (c, t) in enumerate(zip(cargs, args)) if not agrees(c, t)]
    return bad


def test_binding_table_matches_header_types():
    """arity, and the class of the return type and of every parameter: a wrong entry would load and run as undefined behaviour"""
    from vae_gp_ode_amd import _lib
    protos = header_prototypes()
    assert sorted(protos) == declared_symbols() and len(protos) >= 100
    assert protos['gpode_version'] == ('char*', []) and protos['gpode_defer_reductions'] == ('void', ['int'])
    assert protos['gpode_cache_sizes'] == ('int', ['int'] * 5 + ['size_t*'] * 2)
    assert protos['gpode_noise_fill'][1][:4] == ['float*', 'long long', 'long long', 'unsigned long long']
    assert signature_mismatches(_lib.SIGNATURES, protos) == []
    # the check reports each kind of wrong entry (on a copy of the table)
    name = 'gpode_sigmoid_loglik_fwd_len'
    res, args = _lib.SIGNATURES[name]
    i_int, i_sz, i_ptr = args.index(ctypes.c_int), args.index(ctypes.c_size_t), args.index(ctypes.c_void_p)
    for wrong, words in (((res, args[:-1]), 'parameters'), ((res, args + [ctypes.c_int]), 'parameters'),
                         ((res, args[:i_sz] + [ctypes.c_int] + args[i_sz + 1:]), 'parameter %d is size_t' % i_sz),
                         ((res, args[:i_int] + [ctypes.c_size_t] + args[i_int + 1:]), 'parameter %d is int' % i_int),
                         ((res, args[:i_int] + [ctypes.c_float] + args[i_int + 1:]), 'parameter %d is int' % i_int),
                         ((res, args[:i_ptr] + [ctypes.c_int] + args[i_ptr + 1:]), 'parameter %d is float*' % i_ptr),
                         ((res, args[:i_int] + [ctypes.c_void_p] + args[i_int + 1:]), 'parameter %d is int' % i_int),
                         ((None, args), 'returns int'), ((ctypes.c_char_p, args), 'returns int')):
        got = signature_mismatches(dict(_lib.SIGNATURES, **{name: wrong}), protos)
        assert len(got) == 1 and got[0].startswith(name) and words in got[0], (wrong, got)
    sizes = dict(_lib.SIGNATURES, gpode_cache_sizes=(ctypes.c_int, [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_int)] * 2))
    assert len(signature_mismatches(sizes, protos)) == 2
    assert len(signature_mismatches({k: v for k, v in _lib.SIGNATURES.items() if k != name}, protos)) == 1
    assert signature_mismatches(dict(_lib.SIGNATURES, gpode_version=(ctypes.c_int, [])), protos) == ['gpode_version: returns char*, the table has c_int']


def test_host_only_entry_points():
    """Entry points that do not touch the GPU: version string, supported-dims table, size queries, errors."""
    from vae_gp_ode_amd import _lib, ops
    lib = _lib.load()
    assert b'gfx950' in lib.gpode_version()
    assert lib.gpode_supported(0, 6, 6) == 1 and lib.gpode_supported(0, 6, 3) == 1 and lib.gpode_supported(1, 6, 6) == 1
    assert lib.gpode_supported(1, 6, 3) == 0 and lib.gpode_supported(0, 7, 5) == 0
    pf, wf = ops.cache_sizes('RBF', 6, 6, 100, 256)
    # 4 feature groups x 6 dims x 2 quads x 64 lanes + 2 inducing groups x 3 quads x 64 lanes (float4) + 36 uniforms
    assert pf == 4 * (4 * 6 * 2 * 64 + 2 * 3 * 64) + 36
    assert wf > 6 * 128 * 128
    try:
        ops.cache_sizes('RBF', 7, 5, 10, 10)
    except _lib.GpodeError as e:
        assert 'no specialisation' in str(e)
    else:
        raise AssertionError('expected GpodeError')


def test_product_path_never_imports_oracle():
    """The oracle is test infrastructure: nothing under vae-gp-ode_amd/ may import it."""
    pkg = os.path.join(ROOT, 'vae-gp-ode_amd')
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith('.py'):
                src = open(os.path.join(dp, f)).read()
                assert not re.search(r'^\s*(from|import)\s+oracle', src, flags=re.M), os.path.join(dp, f)
