"""Host side of the MLA form switch (lmdeploy_amd.mla): the refusal of an unknown form and the 'auto' rule."""
import pytest

from lmdeploy_amd import mla


def test_unknown_form_is_refused_before_the_library_is_touched():
    with pytest.raises(ValueError, match="form must be one of .*'expanded'.*got 'flash'"):
        mla.mla_forward(*[None] * 9, softmax_scale=1.0, form='flash')   # any use of an argument would raise something else


@pytest.mark.parametrize('q_len, want', [(1, 'absorbed'), (mla.AUTO_EXPANDED_MIN_Q_LEN - 1, 'absorbed'),
                                         (mla.AUTO_EXPANDED_MIN_Q_LEN, 'expanded'), (4096, 'expanded')])
def test_auto_rule(q_len, want):
    assert mla.pick_form('auto', q_len) == want
    assert mla.pick_form('absorbed', q_len) == 'absorbed' and mla.pick_form('expanded', q_len) == 'expanded'
