// lumix_compat_texmips.h — what GpuTextureCompressor::compressWithMips reads besides tests/cpp/lumix_compat_texcomp.h in a standalone
// build: an Options shape with the two members of TextureCompressor::Options that steer the chain (render_plugins.cpp:77-83). The Input
// shape is lumix_compat_texcomp.h's, which already has is_srgb.
#pragma once

#include "lumix_compat_texcomp.h"

namespace Lumix {

struct TexMipsCompatOptions {
	bool compress = true;
	bool generate_mipmaps = false;
	bool stochastic_mipmap = false;
	float scale_coverage_ref = -0.5f;
};

} // namespace Lumix
