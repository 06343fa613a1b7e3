// Forwarding header for dvo_core/include/dvo/visualization/async_point_cloud_builder.h: the types live in the MI355X adaptor.
#ifndef DVO_AMD_COMPAT_VISUALIZATION_ASYNC_POINT_CLOUD_BUILDER_H_
#define DVO_AMD_COMPAT_VISUALIZATION_ASYNC_POINT_CLOUD_BUILDER_H_
#include "../../../dvo_amd/point_cloud.hpp"
#endif
