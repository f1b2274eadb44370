"""opticalflow_amd - MI355X-native variational optical flow (drop-in for the hot path of
kursawe/OpticalFlow's ``source/optical_flow.py::variational_optical_flow``)."""
from .optical_flow import variational_optical_flow, vary_regularisation, make_fake_data_frame, blur_movie, downsample_movie, conduct_opencv_flow  # noqa: F401
from .optical_flow import calcOpticalFlowFarneback, OPTFLOW_USE_INITIAL_FLOW, OPTFLOW_FARNEBACK_GAUSSIAN  # noqa: F401
from .optical_flow import correct_intensity_change, intensity_histograms  # noqa: F401
from .optical_flow import convert_PIV_result, upsample_PIV_vectors  # noqa: F401
from .optical_flow import conduct_piv, conduct_piv_flow, piv_grid  # noqa: F401

__version__ = "0.1.0"
