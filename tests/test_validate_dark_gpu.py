"""GPU test of eld_amd.validate with the sensor's own noise as a model (letter D): for every bias frame, synthesis that reads the session's
OTHER bias frames lies closer to the real frame than shot noise alone, the rows are marked, and flat pairs report nothing for such models."""
import numpy as np
import pytest

from eld_amd import validate as V

pytestmark = pytest.mark.gpu

BLACK, WHITE, BAYER = [512.0, 520.0, 500.0, 531.0], 16383, [[0, 1], [3, 2]]
KS = (0.8, 3.0)
SIGMA = (3.0, 5.0)               # Gaussian read noise of the two sessions, DN
PACKED = (4, 32, 48)             # 64 x 96 mosaics


def _mint(F=4):
    import torch
    sat = WHITE - max(BLACK)
    sessions, frames = [], []
    for s in range(2):
        prm = {'K': KS[s], 'g_scale': SIGMA[s], 'tl_lambda': 0.0, 'tl_scale': 0.0, 'row_scale': 0.0, 'color_bias': [0.0] * 4}
        bias = torch.stack([V.synthesize_codes(None, prm, 'Pg', 'bayer', 77, 1000 * s + f, WHITE, BLACK, shape=PACKED) for f in range(F)])
        clean = np.full(PACKED, 2000.0 / sat, np.float32)
        flats = torch.stack([V.synthesize_codes(clean, prm, 'Pg', 'bayer', 77, 900000 + 10 * s + d, WHITE, BLACK) for d in range(2)])[None]
        sessions.append({'iso': 100 * (s + 1), 'bias': bias.cpu().numpy(), 'flats': flats.cpu().numpy()})
        frames += [{'session': s, 'iso': 100 * (s + 1), 'K': KS[s], 'lambda': 0.0, 'G_scale': 0.0, 'R_scale': 0.0, 'g_scale': SIGMA[s],
                    'color_bias': np.zeros(4)} for _ in range(F)]
    return sessions, {'frames': frames, 'K': np.array(KS)}


def test_dark_frames_beat_shot_noise_alone(eld_lib):
    sessions, diag = _mint()
    assert sessions[0]['bias'].shape == (4, 64, 96)
    rep = V.validate_camera(sessions, BAYER, BLACK, WHITE, models=['P', 'Pg', 'PD'], source='frames', diag=diag)
    for s in rep['sessions']:
        assert len(s['frames']) == 4
        for fr in s['frames']:
            m = fr['models']
            print('kl P %.4f  Pg %.4f  PD %.4f  floor(PD) %.4f' % (m['P']['kl'], m['Pg']['kl'], m['PD']['kl'], m['PD']['floor']))
            assert m['PD']['kl'] < m['P']['kl']
            assert m['PD']['dark'] == 'leave-one-out' and 'dark' not in m['P'] and 'dark' not in m['Pg']
            assert np.isfinite(m['PD']['kl']) and np.isfinite(m['PD']['floor']) and len(m['PD']['kl_groups']) == 4
        for pr in s['flats']:
            assert pr['models']['PD']['kl_flat'] is None and np.isfinite(pr['models']['Pg']['kl_flat'])
        assert s['means']['PD']['kl_flat'] is None and np.isfinite(s['means']['PD']['kl'])
    assert rep['means']['PD']['kl_flat'] is None and rep['means']['PD']['dark'] == 'leave-one-out'
    assert np.isfinite(rep['means']['Pg']['kl_flat']) and rep['best'] in ('Pg', 'PD')
    V.to_jsonable(rep)


def test_single_bias_frame_session_is_refused(eld_lib):
    sessions, diag = _mint(F=2)
    sessions[1]['bias'] = sessions[1]['bias'][:1]
    diag['frames'] = diag['frames'][:3]
    with pytest.raises(ValueError, match='single bias frame'):
        V.validate_camera(sessions, BAYER, BLACK, WHITE, models=['P', 'PD'], source='frames', diag=diag)
    rep = V.validate_camera(sessions, BAYER, BLACK, WHITE, models=['P'], source='frames', diag=diag)      # without D one frame is enough, as before
    assert len(rep['sessions'][1]['frames']) == 1
