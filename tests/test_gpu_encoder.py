"""CIF / CAF target encoders on the device (pp_encode_cif, pp_encode_caf): every fixture of
the reference bit for bit into a sentinel-filled buffer, batches (equal sizes, mixed sizes,
more workgroups than CUs, planes around the 256 cells one workgroup takes, a 161x161 field)
against the host twin, buffer reuse, no stream synchronisation, and the round trip through
the decoder."""
import numpy as np
import pytest

import encoder_util as eu
import golden_util as gu
import oracle
from openpifpaf_amd import _lib, constants, encoder, synthetic

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

RUNS = eu.fixture_runs()
SENTINEL = 12345.678  # no tensor holds it: intensities are 0, 1, NaN; the rest are small
TAIL = 64


def _elems(enc, sizes):
    stride = int(enc.rescaler.stride)
    fn = getattr(_lib.load(), 'pp_encode_%s_output_size' % enc._name)
    return sum(fn((h - 1) // stride + 1, (w - 1) // stride + 1, enc._n_fields())
               for h, w in sizes)


def _encode(enc, scenes):
    """enc.batch into a sentinel-filled buffer: the results as NumPy, after checking that
    every element of the batch was written and nothing behind it."""
    sizes = [s[0] for s in scenes]
    n = _elems(enc, sizes)
    out = torch.full((n + TAIL,), SENTINEL, dtype=torch.float32, device='cuda')
    got = enc.batch(sizes, [s[1] for s in scenes], [s[2] for s in scenes], out=out)
    host = out.cpu().numpy()
    assert not (host[:n] == np.float32(SENTINEL)).any()
    assert (host[n:] == np.float32(SENTINEL)).all()
    if isinstance(got, tuple):
        return tuple(t.cpu().numpy() for t in got)
    return [tuple(t.cpu().numpy() for t in per) for per in got]


def _fixture_encoder(name, which, stride):
    fx = eu.load_fixture(name)
    cif, caf = eu.encoders(eu.fixture_case(fx), stride)
    return fx, (cif if which == 'cif' else caf)


@pytest.mark.parametrize('name,which,stride', RUNS, ids=['%s-%s-s%d' % r for r in RUNS])
def test_device_matches_reference(name, which, stride):
    fx, enc = _fixture_encoder(name, which, stride)
    got = _encode(enc, [eu.fixture_scene(fx)])
    want = eu.expected(fx, which, stride)
    assert len(got) == len(want)
    for g, e in zip(got, want):
        assert eu.same_bits(g[0], e)


DEFAULTS = ('two', 'overlap', 'border', 'few', 'empty', 'crowd_only')  # one set of options


@pytest.mark.parametrize('which', ['cif', 'caf'])
@pytest.mark.parametrize('stride', eu.STRIDES)
def test_one_batch_of_the_equal_size_cases(which, stride):
    _, enc = _fixture_encoder('two', which, stride)
    got = _encode(enc, [eu.fixture_scene(eu.load_fixture(n)) for n in DEFAULTS])
    assert isinstance(got, tuple)
    for i, name in enumerate(DEFAULTS):
        for g, e in zip(got, eu.expected(eu.load_fixture(name), which, stride)):
            assert g.shape[0] == len(DEFAULTS) and eu.same_bits(g[i], e)


def _people(n, h, w, seed):
    rng = np.random.default_rng(seed)
    return [eu.ann(eu.person(rng.uniform(0.1, 0.9) * w, rng.uniform(0.0, 0.5) * h,
                             rng.uniform(0.02, 0.08) * h, seed * 100 + i)) for i in range(n)]


def _against_twin(enc, scenes):
    got = _encode(enc, scenes)
    want = enc.batch_cpu([s[0] for s in scenes], [s[1] for s in scenes], [s[2] for s in scenes],
                         n_threads=8)
    assert type(got) is type(want)
    if isinstance(got, tuple):
        got, want = [got], [want]
    assert len(got) == len(want)
    for g_img, w_img in zip(got, want):
        for g, e in zip(g_img, w_img):
            assert eu.same_bits(g, e)
    return got


@pytest.mark.parametrize('which', ['cif', 'caf'])
def test_mixed_sizes_and_annotation_counts(which):
    """Images of 0, 1, 2 and 7 annotations and a crowd-only one, five sizes, one launch."""
    _, enc = _fixture_encoder('two', which, 8)
    scenes = [((161, 193), [], {}),
              ((97, 130), _people(1, 97, 130, 1), {'valid_area': np.array([3.0, 9.0, 100.0, 80.0])}),
              ((200, 64), _people(2, 200, 64, 2), {}),
              ((240, 321), _people(7, 240, 321, 3) + [eu.crowd((100.0, 50.0, 90.0, 70.0))], {}),
              ((33, 40), [eu.crowd((5.0, 5.0, 20.0, 10.0))], {})]
    got = _against_twin(enc, scenes)
    assert isinstance(got, list) and len(got) == 5
    assert (got[3][0] == 1.0).any() and np.isnan(got[4][0]).any()


@pytest.mark.parametrize('which', ['cif', 'caf'])
def test_more_workgroups_than_compute_units(which):
    """64 copies of a 13x17 field: 64 x K (or C) workgroups."""
    _, enc = _fixture_encoder('two', which, 8)
    scene = ((100, 132), _people(3, 100, 132, 5), {})
    got = _against_twin(enc, [scene] * 64)[0]
    assert got[0].shape[:1] == (64,) and got[0].shape[-2:] == (13, 17)
    for t in got:
        assert (t.view(np.uint32) == t[:1].view(np.uint32)).all()


@pytest.mark.parametrize('which', ['cif', 'caf'])
def test_planes_around_one_workgroup_and_a_large_field(which):
    """A workgroup takes 256 consecutive cells of a plane and holds no plane in LDS, so the
    sizes at which the launch changes shape are 255, 256 and 257 cells per plane (one
    workgroup, one full, two); the 161x161 field (641 px at stride 4) has 102 per plane, with
    patches and limbs across every one of their edges."""
    _, enc = _fixture_encoder('two', which, 4)
    for h, w in ((15 * 4, 17 * 4), (16 * 4, 16 * 4), (1, 257 * 4)):
        people = _people(3, max(h, 40), w, 7)
        got = _against_twin(enc, [((h, w), people, {})])[0]
        assert got[0].shape[-2] * got[0].shape[-1] in (255, 256, 257)
    people = [eu.ann(eu.person(320.0, 40.0, 55.0, 11)), eu.ann(eu.person(200.0, 300.0, 30.0, 12)),
              eu.ann(eu.person(500.0, 200.0, 40.0, 13)), eu.crowd((0.0, 500.0, 641.0, 100.0))]
    got = _against_twin(enc, [((641, 641), people, {'valid_area': np.array([8.0, 0.0, 620.0, 630.0])})])[0]
    assert got[0].shape[-2:] == (161, 161) and (got[0] == 1.0).sum() > 100


@pytest.mark.parametrize('which', ['cif', 'caf'])
def test_consecutive_calls_reuse_the_buffers(which):
    fx, enc = _fixture_encoder('two', which, 8)
    big = [eu.fixture_scene(eu.load_fixture(n)) for n in ('two', 'overlap', 'border')]
    small = [eu.fixture_scene(eu.load_fixture('few'))]

    def run(scenes):
        return enc.batch([s[0] for s in scenes], [s[1] for s in scenes], [s[2] for s in scenes])
    first = run(big)
    ptr = (enc._out.data_ptr(), enc._tab.data_ptr())
    for i, name in enumerate(('two', 'overlap', 'border')):
        for g, e in zip(first, eu.expected(eu.load_fixture(name), which, 8)):
            assert eu.same_bits(g[i].cpu().numpy(), e)
    second = run(small)
    assert (enc._out.data_ptr(), enc._tab.data_ptr()) == ptr
    for g, e in zip(second, eu.expected(eu.load_fixture('few'), which, 8)):
        assert eu.same_bits(g[0].cpu().numpy(), e)
    third = enc.batch([big[0][0]], [big[0][1]], [big[0][2]], fresh=True)
    assert third[0].data_ptr() != ptr[0]
    for g, e in zip(third, eu.expected(fx, which, 8)):
        assert eu.same_bits(g[0].cpu().numpy(), e)


def test_no_call_synchronises_the_stream():
    """With about 20 ms of work queued in front, both encoders return while it still runs."""
    fx = eu.load_fixture('two')
    cif, caf = eu.encoders(eu.fixture_case(fx), 8)
    size, anns, meta = eu.fixture_scene(fx)
    cif.batch([size], [anns], [meta])  # buffers allocated, library loaded
    caf.batch([size], [anns], [meta])
    torch.cuda.synchronize()
    torch.cuda._sleep(50_000_000)
    queued = torch.cuda.Event()
    queued.record()
    a = cif.batch([size] * 4, [anns] * 4, [meta] * 4)
    b = caf.batch([size] * 4, [anns] * 4, [meta] * 4)
    still_running = not queued.query()
    torch.cuda.synchronize()
    assert still_running
    for got, which in ((a, 'cif'), (b, 'caf')):
        for g, e in zip(got, eu.expected(fx, which, 8)):
            assert eu.same_bits(g[3].cpu().numpy(), e)


def test_call_has_the_reference_signature():
    class Visualizer:
        calls = []

        def processed_image(self, image):
            self.calls.append(('image', image.shape))

        def targets(self, fields, *, keypoint_sets):
            self.calls.append(('targets', len(fields), keypoint_sets.shape))
    fx = eu.load_fixture('two')
    cif, caf = eu.encoders(eu.fixture_case(fx), 4)
    size, anns, meta = eu.fixture_scene(fx)
    image = np.zeros((3,) + size, np.float32)
    fields = cif(image, anns, meta)
    assert all(t.is_cuda for t in fields)
    for g, e in zip(fields, eu.expected(fx, 'cif', 4)):
        assert eu.same_bits(g.cpu().numpy(), e)
    caf.visualizer = Visualizer()
    fields = caf(image, anns, meta)
    assert Visualizer.calls == [('image', image.shape), ('targets', 5, (2, 17, 3))]
    for g, e in zip(fields, eu.expected(fx, 'caf', 4)):
        assert eu.same_bits(g.cpu().numpy(), e)
    assert np.array_equal(anns[0]['keypoints'], fx['ann_keypoints'][0])


@pytest.mark.parametrize('name', ['two', 'overlap'])
def test_round_trip_by_two_routes(name):
    """Route one: the device targets through fields_from_targets, decoded by CifCaf.  Route
    two: the reference fixture's targets through the same helper, decoded by the oracle.
    Byte-equal records."""
    from openpifpaf_amd import decoder
    mode = {'mode': 'eval', 'connection_method': 'blend', 'greedy': 0}
    gu.configure_decoder(decoder, mode)
    fx = eu.load_fixture(name)
    cif_enc, caf_enc = eu.encoders(eu.fixture_case(fx), 8)
    size, anns, meta = eu.fixture_scene(fx)
    cif, caf = synthetic.fields_from_targets(cif_enc.batch([size], [anns], [meta]),
                                             caf_enc.batch([size], [anns], [meta]))
    assert cif.shape[1:3] == (17, 5) and caf.shape[1:3] == (19, 9)
    cc = decoder.CifCaf(decoder.FieldConfig(), keypoints=constants.COCO_KEYPOINTS,
                        skeleton=constants.COCO_PERSON_SKELETON)
    recs, offsets, _ = cc.decode_records(cif, caf)
    ref_cif, ref_caf = synthetic.fields_from_targets(
        tuple(np.array(t)[None] for t in eu.expected(fx, 'cif', 8)),
        tuple(np.array(t)[None] for t in eu.expected(fx, 'caf', 8)))
    ref = oracle.decode(ref_cif[0].cpu().numpy(), ref_caf[0].cpu().numpy(),
                        constants.COCO_PERSON_SKELETON, gu.case_config(mode))
    got = recs[offsets[0]:offsets[1]]
    assert len(got) == len(ref) >= 2
    for field in ('data', 'joint_scales', 'n_decoding', 'decoding_pairs', 'decoding_xyv'):
        assert np.array_equal(got[field], ref[field]), field
